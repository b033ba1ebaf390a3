"""What a change of sample rate costs ("Output rates").

    python scripts/bench_resample.py [--repeats 50] [--out FILE]

Four shapes: 8 x 64000 at 16 kHz to 48 kHz and to 44.1 kHz (a generated batch), one 60 s clip to 48 kHz with normalisation and PCM (what
--synthesize --output_rate 48000 adds), and 8 x 176400 at 44.1 kHz to 16 kHz (recordings brought to the model's rate).  For each, on the
same device in the same process and alternating: gs_resample (the entry point on preallocated buffers, HIP events around every call)
and a torch restatement of the same sum -- gather [n_out, taps] samples per row with a precomputed index, multiply by the precomputed tap
rows, sum over the taps (index and tap rows are built outside the timed region; normalisation and PCM, where asked for, as torch ops).
Reported per shape: median / min / max device ms of both (one call between two events: for gs_resample that includes the launch
latency of its one or two kernels), gs_resample's ms per call in bursts of 20 back-to-back calls, their largest difference, and the
two roofs the kernel is held against -- (n_in + n_out) * 4 bytes per row over the measured HBM copy rate, and n_out * taps FMAs per row
over the fp32 vector peak.
Needs a GPU; prints one JSON object.
"""
import argparse
import ctypes
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_BYTES_PER_S = 6.29e12      # float4 copy, measured (8.0e12 by the datasheet)
FP32_FMA_PER_S = 157.3e12 / 2  # vector peak, datasheet

SHAPES = [dict(name="batch 8 x 64000, 16000 -> 48000", rows=8, n_in=64000, rates=(16000, 48000), tail=False),
          dict(name="batch 8 x 64000, 16000 -> 44100", rows=8, n_in=64000, rates=(16000, 44100), tail=False),
          dict(name="60 s clip, 16000 -> 48000, normalise + PCM", rows=1, n_in=960000, rates=(16000, 48000), tail=True),
          dict(name="batch 8 x 176400, 44100 -> 16000", rows=8, n_in=176400, rates=(44100, 16000), tail=False)]


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
        raise SystemExit("bench_resample.py measures on the GPU: no device found")
    from gansynth_amd import _lib, kernels
    torch.cuda.set_device(0)
    K = kernels.get()
    results = []
    for shape in SHAPES:
        rows, n_in, (rate_in, rate_out), tail = shape["rows"], shape["n_in"], shape["rates"], shape["tail"]
        design, table = K.resample_design(rate_in, rate_out, "cuda")
        up, down, taps = design.up, design.down, design.taps
        n_out = int(K.lib.gs_resample_out_len(ctypes.byref(design), n_in))
        x = (torch.rand(rows, n_in, device="cuda", generator=torch.Generator("cuda").manual_seed(0)) * 2 - 1) * (1.0 if tail else 0.3)
        out = torch.empty(rows, n_out, device="cuda")
        pcm = torch.empty(rows, n_out, dtype=torch.int16, device="cuda") if tail else None
        peak = torch.empty(rows, device="cuda") if tail else None
        ws = torch.empty(max(K.lib.gs_resample_workspace_bytes(ctypes.byref(design), rows, n_in), 256), dtype=torch.uint8, device="cuda")

        def kernel():
            _lib.check(K.lib.gs_resample(ctypes.byref(design), table.data_ptr(), x.data_ptr(), rows, n_in, n_in, 1 if tail else 0, out.data_ptr(),
                                         None if pcm is None else pcm.data_ptr(), None if peak is None else peak.data_ptr(), ws.data_ptr(),
                                         ws.numel(), kernels._stream()), "gs_resample")

        # the restatement's constants: the input index of every (output, tap) in a zero-padded row, and every output's tap row
        j = torch.arange(n_out, device="cuda", dtype=torch.int64)
        index = ((j * down) // up)[:, None] + 1 + torch.arange(taps, device="cuda")[None, :] + (taps - taps // 2)
        tap_rows = table.view(up, -1)[:, :taps][(j * down) % up].contiguous()
        held = {}

        def restatement():
            padded = torch.nn.functional.pad(x, (taps, taps))
            y = (padded[:, index] * tap_rows[None]).sum(dim=2)
            if tail:
                top = y.abs().amax(dim=1, keepdim=True)
                y = torch.where(top > 1, y / top, y)
                held["pcm"] = (y * 32768).round().clamp(-32768, 32767).to(torch.int16)
            held["y"] = y

        for _ in range(5):
            kernel()
            restatement()
        difference = float((out - held["y"]).abs().max())
        kernel_ms, torch_ms = [], []
        for _ in range(5):   # alternating blocks: other work shares the machine
            kernel_ms += timed(kernel, args.repeats // 5)
            torch_ms += timed(restatement, max(args.repeats // 25, 1))
        burst = stats([ms / 20 for ms in timed(lambda: [kernel() for _ in range(20)], 10)])
        bytes_moved = rows * (n_in + n_out) * 4
        fmas = rows * n_out * taps
        k = stats(kernel_ms)
        results.append(dict(shape=shape["name"], rows=rows, n_in=n_in, n_out=n_out, up=up, down=down, taps=taps, tail=tail,
                            gs_resample_ms=k, gs_resample_burst_ms=burst, torch_restatement_ms=stats(torch_ms), largest_difference=difference,
                            bytes=bytes_moved, fmas=fmas, hbm_roof_ms=bytes_moved / HBM_BYTES_PER_S * 1e3, fma_roof_ms=fmas / FP32_FMA_PER_S * 1e3,
                            gb_per_s=bytes_moved / k["median"] / 1e6, gfma_per_s=fmas / k["median"] / 1e6))
        del index, tap_rows, held
    result = dict(repeats=args.repeats, hbm_bytes_per_s=HBM_BYTES_PER_S, fp32_fma_per_s=FP32_FMA_PER_S, shapes=results)
    print(json.dumps(result))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
