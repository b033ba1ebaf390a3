"""What the limiter stage costs ("Limiter").

    python scripts/bench_limiter.py [--repeats 50] [--out FILE]

Two clips -- a minute of stereo at 48 kHz and a 4 s mono note at 16 kHz -- at the look-aheads W = 240 and W = 2048.  For each, on the same
device in the same process and alternating: gs_limit (the entry point on preallocated buffers with PCM, peak and least gain, HIP events
around every call: its two launches and their launch latencies) and a torch restatement of the same result -- the scaling, the envelope over
the rows, the ratio, the sliding minimum as -max_pool1d(-r) over W + 1 on the clip padded with ones, the sliding mean as avg_pool1d over
W + 1, the product, the clamp and the PCM as torch ops.  Reported per case: median / min / max device ms of each, gs_limit's ms per call in
bursts of 10 back-to-back calls, the largest difference of the two results, and the stage's algorithmic bytes -- 4 * rows * n read,
(4 + 2) * rows * n written -- over the measured HBM copy rate.
Needs a GPU; prints one JSON object.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_BYTES_PER_S = 6.29e12      # float4 copy, measured (8.0e12 by the datasheet)

CLIPS = [dict(name="60 s stereo at 48 kHz", rows=2, n=2880000), dict(name="4 s mono at 16 kHz", rows=1, n=64000)]
LOOKAHEADS = (240, 2048)


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


def stats(ms):
    ms = sorted(ms)
    return dict(median=ms[len(ms) // 2], min=ms[0], max=ms[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_limiter.py measures on the GPU: no device found")
    from gansynth_amd import _lib, kernels
    torch.cuda.set_device(0)
    K = kernels.get()
    d, c = 1.4, 10.0 ** (-1.0 / 20)
    results = []
    for clip in CLIPS:
        rows, n = clip["rows"], clip["n"]
        x = (torch.rand(rows, n, device="cuda", generator=torch.Generator("cuda").manual_seed(0)) * 2 - 1)
        x *= torch.rand(1, n, device="cuda", generator=torch.Generator("cuda").manual_seed(1)) ** 4      # mostly quiet, some peaks
        out = torch.empty(rows, n, device="cuda")
        pcm = torch.empty(n, rows, dtype=torch.int16, device="cuda")
        peak, gain = torch.empty(1, device="cuda"), torch.empty(1, device="cuda")
        ws_bytes = int(K.lib.gs_limit_workspace_bytes(rows, n))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
        for W in LOOKAHEADS:
            def kernel():
                _lib.check(K.lib.gs_limit(x.data_ptr(), rows, n, n, d, c, W, out.data_ptr(), n, pcm.data_ptr(), peak.data_ptr(), gain.data_ptr(),
                                          ws.data_ptr(), ws_bytes, kernels._stream()), "gs_limit")

            held = {}

            def restatement():
                y = x * d
                a = y.abs().amax(dim=0)
                r = torch.where(a > c, c / a, torch.ones_like(a))
                padded = torch.nn.functional.pad(r[None, None], (W, W), value=1.0)
                m = -torch.nn.functional.max_pool1d(-padded, W + 1, stride=1)
                g = torch.nn.functional.avg_pool1d(m, W + 1, stride=1)[0, 0]
                held["out"] = (g * y).clamp(-c, c)
                held["pcm"] = (held["out"] * 32768).round().clamp(-32768, 32767).to(torch.int16).t().contiguous()

            for _ in range(3):
                kernel()
                restatement()
            difference = float((out - held["out"]).abs().max())
            kernel_ms, torch_ms = [], []
            for _ in range(5):   # alternating blocks: other work shares the machine
                kernel_ms += timed(kernel, args.repeats // 5)
                torch_ms += timed(restatement, max(args.repeats // 25, 1))
            burst = stats([ms / 10 for ms in timed(lambda: [kernel() for _ in range(10)], 5)])
            k = stats(kernel_ms)
            bytes_moved = 4 * rows * n + (4 + 2) * rows * n
            tiles = -(-n // _lib.LIMIT_TILE)
            results.append(dict(clip=clip["name"], rows=rows, n=n, lookahead=W, tiles=tiles, gs_limit_ms=k, gs_limit_burst_ms=burst,
                                torch_restatement_ms=stats(torch_ms), largest_difference=difference, peak=float(peak), min_gain=float(gain),
                                bytes=bytes_moved, hbm_roof_ms=bytes_moved / HBM_BYTES_PER_S * 1e3, gb_per_s=bytes_moved / k["median"] / 1e6,
                                halo_read_bytes=tiles * 2 * W * rows * 4, lds_passes=2 * ((W + 1).bit_length() - 1)))
            del held
    result = dict(repeats=args.repeats, hbm_bytes_per_s=HBM_BYTES_PER_S, pre_gain=d, ceiling=c, cases=results)
    print(json.dumps(result))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
