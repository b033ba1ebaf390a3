"""What the averaged generator costs (DESIGN.md "Averaged generator"): ms per iteration with averaging off and on -- full size, bf16, batch 8,
graphs on (the one-graph iteration) -- and the time of one gs_ema_step, one gs_swap_f32 and one Adam step over the generator's flat buffer.

    python scripts/bench_ema.py [--runs 3] [--steps 60] [--out profiles/ema_bench.json]

The two settings alternate, `--runs` of each; every run is a fresh child process under its own time limit, and the script stops at the first
non-zero status.  GS_EMA_BEFORE_REFRESH=1 in the environment times the other position of the node.  Kernel launches per iteration are counted
from the eager launch sequence (torch.profiler), as bench.py counts them.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_GBPS = 8000.0   # MI355X peak (bench.py)


def worker(args):
    import torch
    import bench
    from gansynth_amd import kernels, variables
    from gansynth_amd.models import GANSynth
    from gansynth_amd.networks import PGGAN
    from gansynth_amd.utils import Dict
    dtype = torch.bfloat16
    variables.set_default_store(variables.VariableStore(device="cuda", seed=0))
    pggan = PGGAN(min_resolution=[2, 16], max_resolution=[128, 1024], min_channels=32, max_channels=256, growing_level=1.0)
    hyper = Dict(generator_learning_rate=8e-4, generator_beta1=0.0, generator_beta2=0.99, discriminator_learning_rate=8e-4,
                 discriminator_beta1=0.0, discriminator_beta2=0.99, mode_seeking_loss_weight=0.1, real_gradient_penalty_weight=5.0,
                 fake_gradient_penalty_weight=0.0, generator_average_decay=args.decay)
    pool = bench.synthetic_pool(8, 0, dtype)
    cursor = [0]

    def real_input_fn():
        _, lab, real = pool[cursor[0] % len(pool)]
        return real, lab

    def fake_input_fn():
        lat, _, _ = pool[cursor[0] % len(pool)]
        cursor[0] += 1
        return lat

    model = GANSynth(pggan.generator, pggan.discriminator, real_input_fn, fake_input_fn, None, hyper, dtype=dtype, use_graphs=True)
    for _ in range(3):
        model.train_step()
    model.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        model.train_step()
    model.synchronize()   # (the last generator step applied: exactly `steps` whole iterations inside)
    ms = (time.perf_counter() - t0) / args.steps * 1e3
    out = {"decay": args.decay, "ms_per_iteration": ms, "steps": args.steps, "one_graph": bool((model._merged or {}).get("fused")),
           "before_refresh": bool(model.ema_before_refresh), "generator_flat_floats": int(model.g_params.flat.numel())}
    if args.count:
        out["kernel_launches_per_iteration"] = bench.count_launches(model)
    if args.micro:
        out["micro"] = micro(kernels.get(), model.g_params.flat.numel())
    print("RESULT " + json.dumps(out), flush=True)


def micro(K, n, sets=4, iters=200):
    """One launch over a buffer of the generator's size: `iters` back-to-back launches inside one event pair, rotating over `sets` sets of
    buffers (4 x 3 x 36 MB: a launch does not find its operands in the 256 MB last-level cache from the launch before)."""
    import torch
    bufs = [[torch.randn(n, device="cuda") for _ in range(4)] for _ in range(sets)]
    for b in bufs:
        b[3].abs_()   # (Adam's v)

    def timed(fn):
        for i in range(2 * sets):
            fn(bufs[i % sets])
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for i in range(iters):
            fn(bufs[i % sets])
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / iters

    rows = {}
    for name, nbytes, fn in (
            ("gs_ema_step", 12, lambda b: K.ema_step(b[0], b[1], 0.001)),
            ("gs_swap_f32", 16, lambda b: K.swap_(b[0], b[1])),
            ("gs_adam_tf_step_zero_grad", 32, lambda b: K.adam_tf_step(b[0], b[1], b[2], b[3], 1e-6, 0.0, 0.99, 1e-8, refresh=False, zero_grad=True))):
        ms = timed(fn)
        rows[name] = {"ms": ms, "bytes_per_element": nbytes, "gbps": n * nbytes / ms / 1e6, "ms_at_hbm_peak": n * nbytes / HBM_GBPS / 1e6}
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--timeout", type=int, default=240, help="seconds, per child process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ema_bench.json"))
    ap.add_argument("--worker", action="store_true", help="(internal) one measurement in this process")
    ap.add_argument("--decay", type=float, default=0.0)
    ap.add_argument("--micro", action="store_true")
    ap.add_argument("--count", action="store_true")
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    runs = {"off": [], "on": []}
    extra = {}
    for i in range(args.runs):
        for name, decay in (("off", 0.0), ("on", 0.999)):
            cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--decay", str(decay), "--steps", str(args.steps)]
            if i == 0:
                cmd += ["--count"] + (["--micro"] if name == "on" else [])
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)   # (a child past its limit is killed: TimeoutExpired ends the script)
            if r.returncode != 0:
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                raise SystemExit(f"bench_ema: the {name} run {i} ended with status {r.returncode}: stopping")
            row = json.loads(next(line for line in r.stdout.splitlines() if line.startswith("RESULT "))[len("RESULT "):])
            runs[name].append(row["ms_per_iteration"])
            for k in ("kernel_launches_per_iteration", "micro"):
                if k in row:
                    extra.setdefault(name, {})[k] = row[k]
            extra.setdefault(name, {}).update(one_graph=row["one_graph"], before_refresh=row["before_refresh"], floats=row["generator_flat_floats"])
            print(f"{name} run {i}: {row['ms_per_iteration']:.4f} ms per iteration", flush=True)
    mean = {k: sum(v) / len(v) for k, v in runs.items()}
    n = extra["on"]["floats"]
    out = {"settings": "full size (2x16 -> 128x1024), bf16, batch 8, graphs on, %d timed iterations per run, runs alternated" % args.steps,
           "ms_per_iteration": runs, "mean_ms": mean, "spread_ms": {k: max(v) - min(v) for k, v in runs.items()},
           "added_ms": mean["on"] - mean["off"], "generator_flat_floats": n,
           "streaming_estimate_ms": n * 12 / HBM_GBPS / 1e6, "node_before_refresh": extra["on"]["before_refresh"],
           "one_graph": [extra["off"]["one_graph"], extra["on"]["one_graph"]],
           "kernel_launches_per_iteration": {k: extra[k].get("kernel_launches_per_iteration") for k in ("off", "on")},
           "micro": extra["on"].get("micro")}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
