#!/usr/bin/env python3
"""Raw int16 samples in against today's path, in ONE run on the same reads: 16 384 reads of 4 000 DAC samples from
synth.make_dac_reads (a channel a read, outliers at --outlier-rate), page-locked memory, default options.  Prints one JSON line
(profiles/events_raw_probe.json):
  A  today's path: rawdtw_signal_to_pa a read on 16 host threads (a counting pass for the offsets, then the conversion into
     the dense page-locked fp32 array), then rawdtw_detect_begin ... rawdtw_detect_end
  B  rawdtw_signal_chunk_table a read on 16 host threads (the offsets), then rawdtw_detect_raw_begin ... rawdtw_detect_end
for each the host stage, the call (begin ... end, host wall time), the launches' device time and the bytes it uploads; the
plain H2D copy of the int16 array alone and of the fp32 array alone; and whether the two paths' events are the same bits.
Each time is the median of --reps runs after a warm-up of at least 200 ms (events_probe.timed).  The host stages' times
(*_host_ms) include the interpreter's cost of one library call a read, which is most of them; *_host_bulk_ms are the same library
functions over the same samples as 16 long reads, one call a thread: the functions' own time.
python scripts/events_raw_probe.py [--chunks N] [--reps R] [--out PATH]
[--profile: a few calls of B alone and nothing else, for rocprofv3 --kernel-trace --stats]"""
import argparse
import ctypes as C
import json
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from events_probe import timed  # noqa: E402

THREADS = 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=16384)
    ap.add_argument("--samples", type=int, default=4000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--outlier-rate", type=float, default=0.001)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch  # (the plain copies; torch's HIP runtime initialises first, as in the tests)

    torch.cuda.init()
    import rawalign_amd as ra
    from rawalign_amd.events import PinnedArray
    from rawalign_amd.rawsig import CHANNEL_DTYPE
    from rawalign_amd.synth import make_dac_reads

    lib = ra.load_library()
    n, S = a.chunks, a.samples
    N = n * S
    raws, chan_np = make_dac_reads(n, S, seed=20240601, outlier_rate=a.outlier_rate)
    raw = PinnedArray(N, np.int16)
    raw.array[:] = np.concatenate(raws)
    del raws
    chan = PinnedArray(n, CHANNEL_DTYPE)
    chan.array[:] = chan_np
    sig = PinnedArray(N, np.float32)                                   # A's dense pA samples
    sig_off, raw_off = PinnedArray(n + 1, np.uint64), PinnedArray(n + 1, np.uint64)
    s_len = PinnedArray(n, np.uint32)
    eoff_a, ev_a = PinnedArray(n + 1, np.uint64), PinnedArray(N, np.float32)
    eoff_b, ev_b = PinnedArray(n + 1, np.uint64), PinnedArray(N, np.float32)
    eng = ra.Engine(0)
    ms = C.c_float()
    pool = ThreadPoolExecutor(THREADS)
    share = [range(t, n, THREADS) for t in range(THREADS)]
    l_sig = np.zeros(n, np.uint64)
    ch_sz = CHANNEL_DTYPE.itemsize

    def on_pool(fn):
        for f in [pool.submit(fn, ks) for ks in share]:
            f.result()

    # -- A: count, offsets, convert into place -------------------------------------------------------------------
    def a_count(ks):
        for k in ks:
            lib.rawdtw_signal_to_pa(chan.ptr + k * ch_sz, S, raw.ptr + 2 * k * S, None, C.cast(l_sig.ctypes.data + 8 * k, C.POINTER(C.c_uint64)))

    def a_write(ks):
        out = C.c_uint64()
        off = sig_off.array
        for k in ks:
            lib.rawdtw_signal_to_pa(chan.ptr + k * ch_sz, S, raw.ptr + 2 * k * S, sig.ptr + 4 * int(off[k]), C.byref(out))

    def a_host():
        on_pool(a_count)
        sig_off.array[0] = 0
        np.cumsum(l_sig, out=sig_off.array[1:n + 1])
        on_pool(a_write)

    def a_call():
        st = lib.rawdtw_detect_begin(eng._ctx, None, n, sig_off.ptr, sig.ptr, eoff_a.ptr, ev_a.ptr, N)
        st = st or lib.rawdtw_detect_end(eng._ctx, C.byref(ms))
        assert st == 0, lib.rawdtw_last_error(eng._ctx)

    # -- B: the chunk table (one chunk a read here: chunk_size = the read), the offsets -------------------------------
    # window k runs from its read's first sample to the next read's: what lies outside [raw_start[0], raw_start[1]) is dropped
    # under the read's own channel either way
    n_ch = np.zeros(n, np.uint32)
    starts = np.zeros((n, 2), np.uint64)

    def b_table(ks):
        for k in ks:
            lib.rawdtw_signal_chunk_table(chan.ptr + k * ch_sz, S, raw.ptr + 2 * k * S, S, 1, C.cast(l_sig.ctypes.data + 8 * k, C.POINTER(C.c_uint64)),
                                          C.cast(n_ch.ctypes.data + 4 * k, C.POINTER(C.c_uint32)), starts.ctypes.data + 16 * k)

    def b_host():
        on_pool(b_table)
        raw_off.array[:n + 1] = np.arange(n + 1, dtype=np.uint64) * np.uint64(S)

    def b_call():
        st = lib.rawdtw_detect_raw_begin(eng._ctx, None, n, raw_off.ptr, raw.ptr, chan.ptr, s_len.ptr, eoff_b.ptr, ev_b.ptr, N)
        st = st or lib.rawdtw_detect_end(eng._ctx, C.byref(ms))
        assert st == 0, lib.rawdtw_last_error(eng._ctx)

    # -- the host stages without the interpreter's share: the same samples as THREADS long reads, one library call a thread
    per = n // THREADS * S
    bulk_l = np.zeros(THREADS, np.uint64)
    bulk_n = np.zeros(THREADS, np.uint32)
    bulk_start = np.zeros((THREADS, per // S + 1), np.uint64)
    bulk_sig = PinnedArray(N, np.float32)

    def u64_at(arr, k):
        return C.cast(arr.ctypes.data + 8 * k, C.POINTER(C.c_uint64))

    def a_bulk_one(t):
        lib.rawdtw_signal_to_pa(chan.ptr, per, raw.ptr + 2 * t * per, None, u64_at(bulk_l, t))
        lib.rawdtw_signal_to_pa(chan.ptr, per, raw.ptr + 2 * t * per, bulk_sig.ptr + 4 * t * per, u64_at(bulk_l, t))

    def b_bulk_one(t):
        lib.rawdtw_signal_chunk_table(chan.ptr, per, raw.ptr + 2 * t * per, S, per // S, u64_at(bulk_l, t),
                                      C.cast(bulk_n.ctypes.data + 4 * t, C.POINTER(C.c_uint32)), bulk_start[t].ctypes.data)

    def bulk(one):
        def f():
            for r in [pool.submit(one, t) for t in range(THREADS)]:
                r.result()
        return f

    def kernel_ms_of(call):
        def f():
            call()
            return ms.value
        return f

    if a.profile:
        b_host()
        for _ in range(5):
            b_call()
        eng.close()
        return

    a_host()
    b_host()
    rec = {"probe": "events_raw", "chunks": n, "samples_per_chunk": S, "raw_samples": N, "outlier_rate": a.outlier_rate, "threads": THREADS,
           "reps": a.reps, "runs": {}}

    def put(name, fn):
        med, runs = timed(fn, a.reps)
        rec[name] = round(med, 4)
        rec["runs"][name] = runs

    # alternate the two paths so that what else the host does falls on both
    put("A_call_ms", a_call)
    put("B_call_ms", b_call)
    put("A_kernel_ms", kernel_ms_of(a_call))
    put("B_kernel_ms", kernel_ms_of(b_call))
    put("A_call_ms_again", a_call)
    put("B_call_ms_again", b_call)
    put("A_host_ms", a_host)
    put("B_host_ms", b_host)
    put("A_host_bulk_ms", bulk(a_bulk_one))
    put("B_host_bulk_ms", bulk(b_bulk_one))
    kept = int(sig_off.array[n])
    # the results: A's and B's events, and B's s_len against A's chunk lengths
    na, nb = int(eoff_a.array[n]), int(eoff_b.array[n])
    canon = lambda x: np.where(np.isnan(x), np.float32(np.nan), x).view(np.uint32)  # noqa: E731
    same = bool(na == nb and np.array_equal(eoff_a.array[:n + 1], eoff_b.array[:n + 1]) and
                np.array_equal(canon(ev_a.array[:na]), canon(ev_b.array[:nb])) and
                np.array_equal(s_len.array[:n].astype(np.uint64), np.diff(sig_off.array[:n + 1])) and
                np.array_equal(l_sig, s_len.array[:n].astype(np.uint64)))
    # the plain copies from page-locked memory, in the same process
    h16, h32 = torch.from_numpy(raw.array[:N]), torch.from_numpy(sig.array[:kept])
    d16 = torch.empty(N, dtype=torch.int16, device="cuda:0")
    d32 = torch.empty(kept, dtype=torch.float32, device="cuda:0")

    def copy(d, h):
        def f():
            d.copy_(h, non_blocking=True)
            torch.cuda.synchronize()
        return f

    put("h2d_int16_ms", copy(d16, h16))
    put("h2d_fp32_ms", copy(d32, h32))
    rec.update({
        "kept_samples": kept, "events": nb, "A_equals_B_bit_for_bit": same,
        "A_upload_bytes": kept * 4 + (n + 1) * 8, "B_upload_bytes": N * 2 + (n + 1) * 8 + n * ch_sz,
        "A_total_ms": round(rec["A_host_ms"] + rec["A_call_ms"], 4), "B_total_ms": round(rec["B_host_ms"] + rec["B_call_ms"], 4),
        "call_saving_ms": round(rec["A_call_ms"] - rec["B_call_ms"], 4), "copy_saving_ms": round(rec["h2d_fp32_ms"] - rec["h2d_int16_ms"], 4),
        "new_launches_ms": round(rec["B_kernel_ms"] - rec["A_kernel_ms"], 4),
    })
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    pool.shutdown()
    eng.close()


if __name__ == "__main__":
    main()
