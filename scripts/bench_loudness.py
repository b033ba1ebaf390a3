"""What the loudness meter costs ("Loudness").

    python scripts/bench_loudness.py [--repeats 50] [--out FILE]

Two clips -- a minute of stereo at 48 kHz and a 4 s mono note at 16 kHz.  For each: gs_loudness (the entry point on preallocated buffers,
HIP events around every call: its three launches and their launch latencies), per call and in bursts of 10 back-to-back calls, next to
  - the HBM roof of its bytes: x is read TWICE (once for the hops' ends from rest, once for the energies; 4 * rows * n each -- the second
    read of a clip this size comes from the Infinity Cache), the two states a hop (64 bytes) are written and read once, 4 bytes a hop leave;
  - the restatement available on the host: scipy.signal.lfilter twice, squares and hop sums in float64 (wall clock, the clip already in
    host memory; no torch restatement of a recursive filter is written -- torch has no such operation and a Python loop over samples is
    not a comparison).
Reported too: the largest difference of the kernel's energies to that restatement relative to the largest energy, and the time of the
tail of a whole --synthesize on the same minute of stereo, device synchronised, wall clock: limiter.apply with PCM (the tail of --limit,
the code the commit before this one had) and loudness.apply with PCM (the tail of --loudness: gs_loudness, the read-back, the gating on the
host, gs_limit, and the second measurement).
Needs a GPU; prints one JSON object.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_BYTES_PER_S = 6.29e12      # float4 copy, measured (8.0e12 by the datasheet)

CLIPS = [dict(name="60 s stereo at 48 kHz", rows=2, n=2880000, rate=48000), dict(name="4 s mono at 16 kHz", rows=1, n=64000, rate=16000)]


def timed(fn, repeats):
    pairs = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        pairs.append((e0, e1))
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in pairs]


def wall(fn, repeats):
    ms = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def stats(ms):
    ms = sorted(ms)
    return dict(median=ms[len(ms) // 2], min=ms[0], max=ms[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_loudness.py measures on the GPU: no device found")
    from scipy import signal
    from gansynth_amd import _lib, kernels, limiter, loudness
    torch.cuda.set_device(0)
    K = kernels.get()
    results = []
    for clip in CLIPS:
        rows, n, rate = clip["rows"], clip["n"], clip["rate"]
        x = (torch.rand(rows, n, device="cuda", generator=torch.Generator("cuda").manual_seed(0)) * 2 - 1)
        x *= torch.rand(1, n, device="cuda", generator=torch.Generator("cuda").manual_seed(1)) ** 4      # mostly quiet, some peaks
        design = K.loudness_design(rate)
        hops = n // design.hop
        energy = torch.empty(rows, hops, device="cuda")
        ws_bytes = int(K.lib.gs_loudness_workspace_bytes(ctypes.byref(design), rows, n))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")

        def kernel():
            _lib.check(K.lib.gs_loudness(ctypes.byref(design), x.data_ptr(), rows, n, n, energy.data_ptr(), hops, ws.data_ptr(), ws_bytes,
                                         kernels._stream()), "gs_loudness")

        (b1, a1), (b2, a2), hop = loudness.k_weighting(rate)
        host = x.cpu().numpy().astype(np.float64)
        held = {}

        def restatement():
            y = signal.lfilter(b2, a2, signal.lfilter(b1, a1, host, axis=-1), axis=-1)
            held["energy"] = (y[:, :hops * hop].reshape(rows, hops, hop) ** 2).sum(axis=2)

        for _ in range(3):
            kernel()
        restatement()
        difference = float(np.abs(energy.cpu().numpy().astype(np.float64) - held["energy"]).max() / held["energy"].max())
        kernel_ms = []
        for _ in range(5):   # in blocks: other work shares the machine
            kernel_ms += timed(kernel, args.repeats // 5)
        burst = stats([ms / 10 for ms in timed(lambda: [kernel() for _ in range(10)], 5)])
        host_ms = []
        for _ in range(3):
            t0 = time.perf_counter()
            restatement()
            host_ms.append((time.perf_counter() - t0) * 1e3)
        k = stats(kernel_ms)
        bytes_moved = 2 * 4 * rows * n + rows * hops * (2 * 64 + 4)
        case = dict(clip=clip["name"], rows=rows, n=n, rate=rate, hop=int(design.hop), hops=hops, chunk=int(design.chunk), lanes=int(design.lanes),
                    gs_loudness_ms=k, gs_loudness_burst_ms=burst, scipy_lfilter_host_ms=stats(host_ms), largest_difference=difference,
                    x_reads=2, bytes=bytes_moved, hbm_roof_ms=bytes_moved / HBM_BYTES_PER_S * 1e3, gb_per_s=bytes_moved / k["median"] / 1e6,
                    lufs=loudness.integrated(energy.cpu().numpy(), hop))
        if rows == 2:   # the tail of a whole --synthesize on this clip
            peak = x.abs().max()
            tail_limit = wall(lambda: limiter.apply(x, rate, ceiling_db=-1.0, drive_db=6.0, peak=peak, want_pcm=True), 10)
            tail_loudness = wall(lambda: loudness.apply(x, rate, -16.0, want_pcm=True), 10)
            case.update(tail_limit_ms=stats(tail_limit), tail_loudness_ms=stats(tail_loudness))
        results.append(case)
    result = dict(repeats=args.repeats, hbm_bytes_per_s=HBM_BYTES_PER_S, cases=results)
    print(json.dumps(result))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
