"""What the reverb stage costs ("Reverb").

    python scripts/bench_reverb.py [--repeats 50] [--out FILE]

Two shapes: a 60 s stereo clip at 48 kHz against a 2 s designed room of two channels (what --synthesize --stereo --output_rate 48000 --reverb 2
adds), and a 4 s mono clip at 16 kHz against a 1 s room.  For each, on the same device in the same process and alternating: gs_fftconv (the
entry point on preallocated buffers with normalisation and PCM, HIP events around every call: its three launches and their launch
latencies), gs_fftconv_prepare (once per impulse response), and a torch restatement of the same result -- torch.fft.rfft of the whole
zero-padded clip, the product with the impulse's rfft (taken outside the timed region), irfft, dry / wet, one peak, the quotient and PCM as
torch ops.  Reported per shape: median / min / max device ms of each, gs_fftconv's ms per call in bursts of 10 back-to-back calls, the
largest difference of the two unnormalised results, and the stage's algorithmic bytes -- the clip read, the result written, read and
written again by the finish, the PCM, the impulse's spectra read once -- over the measured HBM copy rate.  The block spectra that pass
between the launches (workspace_bytes) and the partition spectra every block re-reads (mac_read_bytes: they come from L2) are reported next
to it: they are traffic of the form chosen, not of the problem.
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

SHAPES = [dict(name="60 s stereo at 48 kHz, 2 s room", rows=2, ir_rows=2, n=2880000, rate=48000, rt60=2.0),
          dict(name="4 s mono at 16 kHz, 1 s room", rows=1, ir_rows=1, n=64000, rate=16000, rt60=1.0)]


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
        raise SystemExit("bench_reverb.py measures on the GPU: no device found")
    from gansynth_amd import _lib, kernels, reverb
    torch.cuda.set_device(0)
    K = kernels.get()
    dry, wet = 0.75, 0.25
    results = []
    for shape in SHAPES:
        rows, ir_rows, n = shape["rows"], shape["ir_rows"], shape["n"]
        h = reverb.design_impulse(shape["rate"], shape["rt60"], channels=ir_rows, seed=0).cuda()
        m = int(h.shape[1])
        n_out = n + m - 1
        design = _lib.GsFftConv()
        _lib.check(K.lib.gs_fftconv_design(n, m, rows, ir_rows, ctypes.byref(design)), "gs_fftconv_design")
        x = (torch.rand(rows, n, device="cuda", generator=torch.Generator("cuda").manual_seed(0)) * 2 - 1)
        stride = (n_out + 3) // 4 * 4
        out = torch.empty(rows, stride, device="cuda")
        pcm = torch.empty(n_out, rows, dtype=torch.int16, device="cuda")
        peak = torch.empty(1, device="cuda")
        spectrum_bytes = int(K.lib.gs_fftconv_spectrum_bytes(ctypes.byref(design)))
        ws_bytes = int(K.lib.gs_fftconv_workspace_bytes(ctypes.byref(design)))
        spectrum = torch.empty(spectrum_bytes, dtype=torch.uint8, device="cuda")
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")

        def prepare():
            _lib.check(K.lib.gs_fftconv_prepare(ctypes.byref(design), h.data_ptr(), m, spectrum.data_ptr(), spectrum_bytes, kernels._stream()),
                       "gs_fftconv_prepare")

        def kernel(normalize=1):
            _lib.check(K.lib.gs_fftconv(ctypes.byref(design), spectrum.data_ptr(), spectrum_bytes, x.data_ptr(), n, dry, wet, normalize, out.data_ptr(),
                                        stride, pcm.data_ptr(), peak.data_ptr(), ws.data_ptr(), ws_bytes, kernels._stream()), "gs_fftconv")

        size = n_out + (n_out & 1)                    # (an even length: irfft gives it back)
        hf = torch.fft.rfft(h, size)                  # once per impulse, like the prepared spectrum
        held = {}

        def restatement(normalize=True):
            y = torch.fft.irfft(torch.fft.rfft(x, size) * hf, size)[:, :n_out] * wet
            y[:, :n] += dry * x
            held["y"] = y
            if normalize:
                top = y.abs().max()
                y = torch.where(top > 1, y / top, y)
                held["pcm"] = (y * 32768).round().clamp(-32768, 32767).to(torch.int16).t().contiguous()

        prepare()
        for _ in range(3):
            kernel()
            restatement()
        kernel(0)
        restatement(False)
        difference = float((out[:, :n_out] - held["y"]).abs().max())
        kernel_ms, torch_ms, prepare_ms = [], [], []
        for _ in range(5):   # alternating blocks: other work shares the machine
            kernel_ms += timed(kernel, args.repeats // 5)
            torch_ms += timed(restatement, max(args.repeats // 25, 1))
            prepare_ms += timed(prepare, max(args.repeats // 25, 1))
        burst = stats([ms / 10 for ms in timed(lambda: [kernel() for _ in range(10)], 5)])
        k = stats(kernel_ms)
        h_spectra = ir_rows * design.partitions * _lib.FFTCONV_BLOCK * 8
        bytes_moved = rows * n * 4 + 3 * rows * n_out * 4 + rows * n_out * 2 + h_spectra
        mac_read = rows * design.blocks * min(design.partitions, design.x_blocks) * 2 * _lib.FFTCONV_BLOCK * 8    # (an upper bound: the edge blocks read fewer)
        results.append(dict(shape=shape["name"], rows=rows, ir_rows=ir_rows, n=n, m=m, n_out=n_out, partitions=design.partitions, blocks=design.blocks,
                            x_blocks=design.x_blocks, gs_fftconv_ms=k, gs_fftconv_burst_ms=burst, gs_fftconv_prepare_ms=stats(prepare_ms),
                            torch_restatement_ms=stats(torch_ms), largest_difference=difference, peak=float(peak), bytes=bytes_moved,
                            hbm_roof_ms=bytes_moved / HBM_BYTES_PER_S * 1e3, gb_per_s=bytes_moved / k["median"] / 1e6, spectrum_bytes=spectrum_bytes,
                            workspace_bytes=ws_bytes, mac_read_bytes=mac_read, mac_read_gb_per_s=mac_read / k["median"] / 1e6))
        del hf, held
    result = dict(repeats=args.repeats, hbm_bytes_per_s=HBM_BYTES_PER_S, dry=dry, wet=wet, shapes=results)
    print(json.dumps(result))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
