"""What the YIN f0 tracker costs on the device ("Pitch tracking on the device").

    python scripts/bench_yin.py [--repeats 10] [--out profiles/yin_bench.json]

Two sizes at the production parameters (W 1024, L 512, hop 256, tau_min 8, threshold 0.15): 64 and 8192 notes of 64000 samples, synthetic
harmonic notes plus noise, in batches of at most 1024 rows (gs_yin_difference writes d, 0.5 MB a note).  For each, on the same device in the
same process and alternating:
  gs_yin_difference and gs_yin_track -- the entries on preallocated buffers, HIP events around every batch, a size's time the sum over its
  batches --
  next to a torch restatement of the difference in the same direct form (frames by unfold, one subtract / square / sum per lag), timed on 64
  notes only: at 8192 its time is stated as 128 times that, and marked as extrapolated.
Reported per size: median / min / max device ms of each, the fp32 vector roof -- 2 W L F rows lane operations (a subtract and a multiply-add per
term) at the datasheet's vector peak of 157.3 TFLOPS, two flops a lane operation -- and each entry's share of it, and the largest relative
deviation of the device's d and of torch's from a float64 d on the first four notes.  Then the wall time `--f0` adds to
`gan_synth_main.py --evaluate --swd --classifier none --synthetic` (8 batches of 8 notes; fresh child processes, alternating, the faster of two
runs each).  Needs a GPU; prints one JSON object.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VECTOR_FLOPS = 157.3e12          # fp32 vector peak of the datasheet
W, L, HOP, TAU_MIN, THRESHOLD, N = 1024, 512, 256, 8, 0.15, 64000
SIZES = [64, 8192]
BATCH = 1024
TORCH_ROWS = 64


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


def notes(rows, seed):
    """[rows, N] fp32 on the device: four harmonics of a pitch in 24 .. 84, a decay, 0.002 noise."""
    g = torch.Generator("cuda").manual_seed(seed)
    t = torch.arange(N, device="cuda", dtype=torch.float32) / 16000.0
    pitch = torch.randint(24, 85, (rows, 1), device="cuda", generator=g).float()
    f0 = 440.0 * 2.0 ** ((pitch - 69.0) / 12.0)
    x = torch.zeros(rows, N, device="cuda")
    for h in range(1, 5):
        amp = (0.2 + 0.8 * torch.rand(rows, 1, device="cuda", generator=g)) / h
        x += amp * torch.sin(2.0 * torch.pi * f0 * h * t[None, :] + 6.28 * torch.rand(rows, 1, device="cuda", generator=g))
    x = x * torch.exp(-t / 1.5)[None, :]
    return 0.7 * x / x.abs().amax(dim=1, keepdim=True) + 0.002 * torch.randn(rows, N, device="cuda", generator=g)


def torch_difference(x, dtype=torch.float32):
    """d [rows, F, L] by torch in the direct form: frames by unfold, one subtract / square / sum per lag."""
    frames = x.to(dtype).unfold(1, W + L, HOP)                 # [rows, F, W + L] (a view)
    head = frames[:, :, :W]
    out = torch.empty(x.shape[0], frames.shape[1], L, dtype=dtype, device=x.device)
    for tau in range(L):
        out[:, :, tau] = ((head - frames[:, :, tau:tau + W]) ** 2).sum(dim=2)
    return out


def evaluate_wall(f0):
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [sys.executable, os.path.join(ROOT, "gan_synth_main.py"), "--evaluate", "--swd", "--classifier", "none", "--synthetic", "--model_dir",
               os.path.join(tmp, "model"), "--batch_size", "8", "--num_generate_batches", "8"] + (["--f0"] if f0 else [])
        t0 = time.perf_counter()
        r = subprocess.run(cmd, cwd=tmp, capture_output=True, text=True, timeout=600)
        wall = time.perf_counter() - t0
        if r.returncode != 0:
            raise SystemExit(f"bench_yin.py: {' '.join(cmd)} failed:\n{r.stderr[-2000:]}")
        return wall


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_yin.py measures on the GPU: no device found")
    from gansynth_amd import _lib, kernels
    torch.cuda.set_device(0)
    K = kernels.get()
    F = int(K.lib.gs_yin_frames(N, W, L, HOP))
    cases, torch_ms_64 = [], None
    for rows in SIZES:
        x = notes(rows, rows)
        batch = min(rows, BATCH)
        d = torch.empty(batch, F, L, device="cuda")
        power = torch.empty(rows, F, device="cuda")
        lag = torch.empty(rows, F, dtype=torch.int32, device="cuda")
        period = torch.empty(rows, F, dtype=torch.float64, device="cuda")
        aper = torch.empty(rows, F, dtype=torch.float64, device="cuda")
        st = kernels._stream()

        def difference():
            for at in range(0, rows, batch):
                _lib.check(K.lib.gs_yin_difference(x[at:].data_ptr(), N, batch, N, W, L, HOP, d.data_ptr(), power[at:].data_ptr(), st), "gs_yin_difference")

        def track():
            for at in range(0, rows, batch):
                _lib.check(K.lib.gs_yin_track(x[at:].data_ptr(), N, batch, N, W, L, HOP, TAU_MIN, THRESHOLD, lag[at:].data_ptr(), period[at:].data_ptr(),
                                              aper[at:].data_ptr(), power[at:].data_ptr(), st), "gs_yin_track")

        fns = dict(difference=difference, track=track)
        if rows == TORCH_ROWS:
            fns["torch_difference"] = lambda: torch_difference(x)
        for _ in range(2):
            for fn in fns.values():
                fn()
        torch.cuda.synchronize()
        lane_ops = 2.0 * W * L * F * rows
        case = dict(rows=rows, n=N, frames=F, batch=batch, lane_operations=lane_ops, vector_roof_ms=lane_ops / (VECTOR_FLOPS / 2.0) * 1e3)
        if rows == TORCH_ROWS:
            exact = torch_difference(x[:4], torch.float64)
            _lib.check(K.lib.gs_yin_difference(x.data_ptr(), N, 4, N, W, L, HOP, d.data_ptr(), power.data_ptr(), st), "gs_yin_difference")
            own = d[:4].double()
            ref = exact.clamp_min(1e-300)
            case["largest_relative_deviation_from_float64_d"] = dict(device=float(((own - exact).abs() / ref)[:, :, 1:].max()),
                                                                     torch=float(((torch_difference(x[:4]).double() - exact).abs() / ref)[:, :, 1:].max()))
            del exact, own, ref
        ms = {name: [] for name in fns}
        for block in range(5):   # alternating blocks: other work shares the machine
            for name, fn in fns.items():
                ms[name] += timed(fn, max(args.repeats // 5, 1))
            print(f"rows {rows}: block {block} timed", file=sys.stderr, flush=True)
        for name in fns:
            case[name + "_ms"] = stats(ms[name])
        if rows == TORCH_ROWS:
            torch_ms_64 = case["torch_difference_ms"]["median"]
        elif torch_ms_64 is not None:
            case["torch_difference_ms_extrapolated_from_64_rows"] = torch_ms_64 * rows / TORCH_ROWS
        for name in ("difference", "track"):
            case[name + "_fraction_of_vector_roof"] = case["vector_roof_ms"] / case[name + "_ms"]["median"]
            case[name + "_lane_operations_per_second"] = lane_ops / case[name + "_ms"]["median"] * 1e3
        cases.append(case)
        del x, d
        torch.cuda.empty_cache()
    walls = {False: [], True: []}
    for _ in range(2):
        for f0 in (False, True):
            walls[f0].append(evaluate_wall(f0))
            print(f"evaluate f0={f0}: {walls[f0][-1]:.2f} s", file=sys.stderr, flush=True)
    result = dict(repeats=args.repeats, vector_flops=VECTOR_FLOPS, parameters=dict(window=W, lags=L, hop=HOP, tau_min=TAU_MIN, threshold=THRESHOLD), cases=cases,
                  evaluate=dict(notes_per_side=64, wall_s_without_f0=walls[False], wall_s_with_f0=walls[True], f0_adds_s=min(walls[True]) - min(walls[False])))
    print(json.dumps(result))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
