"""What the true-peak detector and the limiter that listens to it cost ("True peak").

    python scripts/bench_true_peak.py [--repeats 50] [--out FILE]

Two clips -- a minute of stereo at 48 kHz and a 4 s mono note at 16 kHz.  For each, on the same device in the same process and alternating:
gs_true_peak with the envelope and the peak, gs_true_peak with the peak alone, gs_limit_env and gs_limit at W = 240 (the entry points on
preallocated buffers, HIP events around every call: their launches and launch latencies), and a torch restatement of the detector that DOES
write the 4x signal -- conv1d of the zero-padded clip with the [4, 1, 68] table, abs, amax over the phases and rows, amax over the clip.
Reported per case: median / min / max device ms of each, the kernels' ms per call in bursts of 10 back-to-back calls, the largest difference
of the two envelopes, and two roofs of the detector: 272 FMAs per sample and row at the fp32 vector rate of the datasheet (157.3 TFLOPS, two
flops an FMA, packed), and its algorithmic bytes -- 4 * rows * n read, 4 * n written -- over the measured HBM copy rate.
Then the tail of `--synthesize --limit -1` on the minute of stereo, host clock around work that ends in a synchronise: limiter.apply with
the PCM, without --true_peak (the peak handed over) and with it (detector with envelope, limiter with envelope, detector on the output).
Needs a GPU; prints one JSON object.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_BYTES_PER_S = 6.29e12      # float4 copy, measured (8.0e12 by the datasheet)
VECTOR_FMA_PER_S = 157.3e12 / 2   # fp32 vector rate of the datasheet: 157.3 TFLOPS
FMA_PER_SAMPLE = 4 * 68

CLIPS = [dict(name="60 s stereo at 48 kHz", rows=2, n=2880000), dict(name="4 s mono at 16 kHz", rows=1, n=64000)]
LOOKAHEAD = 240


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


def host_ms(fn, repeats):
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_true_peak.py measures on the GPU: no device found")
    from gansynth_amd import _lib, kernels, limiter, true_peak
    torch.cuda.set_device(0)
    K = kernels.get()
    d, c = 1.4, 10.0 ** (-1.0 / 20)
    table = K.resample_design(1, _lib.TRUE_PEAK_OVERSAMPLE, "cuda")[1]
    weight = table.view(4, 1, 68)
    results = []
    for clip in CLIPS:
        rows, n = clip["rows"], clip["n"]
        x = (torch.rand(rows, n, device="cuda", generator=torch.Generator("cuda").manual_seed(0)) * 2 - 1)
        x *= torch.rand(1, n, device="cuda", generator=torch.Generator("cuda").manual_seed(1)) ** 4      # mostly quiet, some peaks
        env, tp = torch.empty(n, device="cuda"), torch.empty(1, device="cuda")
        out = torch.empty(rows, n, device="cuda")
        pcm = torch.empty(n, rows, dtype=torch.int16, device="cuda")
        peak, gain = torch.empty(1, device="cuda"), torch.empty(1, device="cuda")
        tws_bytes, lws_bytes = int(K.lib.gs_true_peak_workspace_bytes(rows, n)), int(K.lib.gs_limit_workspace_bytes(rows, n))
        tws, lws = torch.empty(tws_bytes, dtype=torch.uint8, device="cuda"), torch.empty(lws_bytes, dtype=torch.uint8, device="cuda")

        def detector():
            _lib.check(K.lib.gs_true_peak(table.data_ptr(), x.data_ptr(), rows, n, n, env.data_ptr(), tp.data_ptr(), tws.data_ptr(), tws_bytes,
                                          kernels._stream()), "gs_true_peak")

        def detector_peak_only():
            _lib.check(K.lib.gs_true_peak(table.data_ptr(), x.data_ptr(), rows, n, n, None, tp.data_ptr(), tws.data_ptr(), tws_bytes,
                                          kernels._stream()), "gs_true_peak")

        tail = (rows, n, n, d, c, LOOKAHEAD, out.data_ptr(), n, pcm.data_ptr(), peak.data_ptr(), gain.data_ptr(), lws.data_ptr(), lws_bytes)

        def limit_env():
            _lib.check(K.lib.gs_limit_env(x.data_ptr(), env.data_ptr(), *tail, kernels._stream()), "gs_limit_env")

        def limit_plain():
            _lib.check(K.lib.gs_limit(x.data_ptr(), *tail, kernels._stream()), "gs_limit")

        held = {}

        def restatement():
            z = torch.nn.functional.conv1d(torch.nn.functional.pad(x[:, None, :], (33, 34)), weight)       # [rows, 4, n]: the 4x signal, written
            held["env"] = torch.maximum(z.abs().amax(dim=(0, 1)), x.abs().amax(dim=0))
            held["peak"] = held["env"].amax()

        fns = dict(gs_true_peak=detector, gs_true_peak_peak_only=detector_peak_only, gs_limit_env=limit_env, gs_limit=limit_plain)
        for _ in range(3):
            for fn in fns.values():
                fn()
            restatement()
        detector()
        difference = float((env - held["env"]).abs().max())
        ms = {name: [] for name in fns}
        torch_ms = []
        for _ in range(5):   # alternating blocks: other work shares the machine
            for name, fn in fns.items():
                ms[name] += timed(fn, args.repeats // 5)
            torch_ms += timed(restatement, max(args.repeats // 25, 1))
        case = dict(clip=clip["name"], rows=rows, n=n, lookahead=LOOKAHEAD, tiles=-(-n // _lib.TRUE_PEAK_TILE), largest_difference=difference,
                    true_peak=float(tp), torch_restatement_ms=stats(torch_ms))
        for name, fn in fns.items():
            case[name + "_ms"] = stats(ms[name])
            case[name + "_burst_ms"] = stats([t / 10 for t in timed(lambda: [fn() for _ in range(10)], 5)])
        fma = FMA_PER_SAMPLE * rows * n
        nbytes = 4 * rows * n + 4 * n
        best = case["gs_true_peak_burst_ms"]["median"]
        case.update(fma=fma, vector_roof_ms=fma / VECTOR_FMA_PER_S * 1e3, bytes=nbytes, hbm_roof_ms=nbytes / HBM_BYTES_PER_S * 1e3,
                    tflops=2 * fma / best / 1e9, fraction_of_vector_roof=fma / VECTOR_FMA_PER_S * 1e3 / best,
                    speedup_over_torch=case["torch_restatement_ms"]["median"] / case["gs_true_peak_ms"]["median"])
        results.append(case)
        del held
        if rows == 2:   # the tail of --synthesize --limit -1, with and without --true_peak
            handed = float(x.abs().max())

            def tail_plain():
                limiter.apply(x, 48000, ceiling_db=-1.0, peak=handed, want_pcm=True)

            def tail_true_peak():
                true_peak.measure(limiter.apply(x, 48000, ceiling_db=-1.0, peak=handed, want_pcm=True, true_peak=True)[0])

            for _ in range(3):
                tail_plain()
                tail_true_peak()
            a, b = [], []
            for _ in range(5):
                a += host_ms(tail_plain, max(args.repeats // 5, 1))
                b += host_ms(tail_true_peak, max(args.repeats // 5, 1))
            driver_tail = dict(clip=clip["name"], limit_host_ms=stats(a), limit_true_peak_host_ms=stats(b))
    result = dict(repeats=args.repeats, hbm_bytes_per_s=HBM_BYTES_PER_S, vector_fma_per_s=VECTOR_FMA_PER_S, pre_gain=d, ceiling=c, cases=results,
                  driver_tail=driver_tail)
    print(json.dumps(result))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
