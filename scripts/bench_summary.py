"""What TensorBoard summaries cost the training loop ("Summaries").

    python scripts/bench_summary.py [--iters 500] [--every 100] [--pairs 2] [--out FILE]

The headline configuration (fully grown 128 x 1024 networks, batch 8, bf16, generated notes through the spectral front end) trained by
GANSynth.train itself, alternately with `save_summary_steps = --every` and with summaries off, `--pairs` times each, every leg a fresh
model in the same process.  A leg runs 2 x `--every` warm-up iterations (captures; with summaries on, the first summary: plans, pinned
buffers) and then `--iters` timed ones, between two log lines -- the trainer's log reads the losses, i.e. waits for the device, in
both kinds of leg alike; a log line comes before the summary of its step, so the window holds iters / every summaries, none of them
the first.  Reported: ms per iteration of every leg, the device time of one summary step (events around the generator pass, the
inverse transform, the quantising launches and the copies), and the writer thread's time per summary step (waiting for
the copy, PNG / WAV encoding, checksums, the write).  Needs a GPU; prints one JSON object.
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def leg(every, iters, summaries, batch, model_dir):
    from gansynth_amd import summary, variables
    from gansynth_amd.dataset import synthetic_nsynth_input_fn
    from gansynth_amd.models import GANSynth
    from gansynth_amd.networks import PGGAN
    from gansynth_amd.utils import Dict

    device = torch.device("cuda", 0)
    torch.manual_seed(0)
    variables.set_default_store(variables.VariableStore(device="cuda", seed=0))
    pggan = PGGAN(min_resolution=[2, 16], max_resolution=[128, 1024], min_channels=32, max_channels=256, growing_level=1.0)
    model = GANSynth(pggan.generator, pggan.discriminator, synthetic_nsynth_input_fn(batch, range(24, 85), device=device, seed=0),
                     lambda: torch.randn(batch, 256, device=device),
                     Dict(waveform_length=64000, sample_rate=16000, spectrogram_shape=[128, 1024], overlap=0.75),
                     Dict(generator_learning_rate=8e-4, generator_beta1=0.0, generator_beta2=0.99, discriminator_learning_rate=8e-4,
                          discriminator_beta1=0.0, discriminator_beta2=0.99, mode_seeking_loss_weight=0.1, real_gradient_penalty_weight=5.0,
                          fake_gradient_penalty_weight=0.0),
                     dtype=torch.bfloat16, use_graphs=True)
    stamps, device_ms, host_s = {}, [], []

    def log(line):
        stamps[model.global_step] = time.perf_counter()   # (the line was formatted from the losses: the device has finished the step)

    if summaries:
        inner = model._summarize

        def timed(*args, **kwargs):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            inner(*args, **kwargs)
            b.record()
            device_ms.append((a, b))
        model._summarize = timed
        values = summary.SummaryWriter._values

        def timed_values(self, items):
            t = time.perf_counter()
            out = list(values(self, items))
            host_s.append(time.perf_counter() - t)
            return out
        summary.SummaryWriter._values = timed_values
    try:
        model.train(model_dir=model_dir, config=None, total_steps=2 * every + iters, save_checkpoint_steps=0,
                    save_summary_steps=every if summaries else None, log_tensor_steps=every, log=log)
    finally:
        if summaries:
            summary.SummaryWriter._values = values
    torch.cuda.synchronize()
    out = dict(summaries=bool(summaries), ms_per_iteration=1e3 * (stamps[2 * every + iters] - stamps[2 * every]) / iters)
    if summaries:
        per = [a.elapsed_time(b) for a, b in device_ms[1:]]          # (the first one warmed up)
        records = host_s[3:]                                          # (three records per summary step: audio, images, scalars)
        out.update(summary_steps_timed=len(per), device_ms_per_summary=sum(per) / max(len(per), 1),
                   host_encode_ms_per_summary=1e3 * sum(records) / max(len(records) / 3, 1),
                   events_file_bytes=sum(os.path.getsize(os.path.join(model_dir, f)) for f in os.listdir(model_dir) if f.startswith("events.")))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=500)
    ap.add_argument("--every", type=int, default=100)
    ap.add_argument("--pairs", type=int, default=2)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_summary.py measures on the GPU: no device found")
    if args.iters % args.every:
        raise SystemExit("--iters must be a multiple of --every")
    legs = []
    for _ in range(args.pairs):
        for summaries in (False, True):
            model_dir = tempfile.mkdtemp(prefix="bench_summary_")
            try:
                legs.append(leg(args.every, args.iters, summaries, args.batch, model_dir))
            finally:
                shutil.rmtree(model_dir, ignore_errors=True)
            print(json.dumps(legs[-1]), flush=True)
    off = [l["ms_per_iteration"] for l in legs if not l["summaries"]]
    on = [l["ms_per_iteration"] for l in legs if l["summaries"]]
    result = dict(config=dict(batch=args.batch, dtype="bf16", resolution=[128, 1024], iters=args.iters, save_summary_steps=args.every),
                  legs=legs, ms_per_iteration_off=sum(off) / len(off), ms_per_iteration_on=sum(on) / len(on),
                  off_spread=max(off) - min(off), on_minus_off_percent=100.0 * (sum(on) / len(on) / (sum(off) / len(off)) - 1.0))
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
