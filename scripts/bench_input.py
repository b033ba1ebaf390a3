"""What input costs a training iteration: the host pipeline (dataset.nsynth_input_fn), the resident bank (bank.bank_input_fn) and a
feed that costs nothing (batches prepared on the device in advance), each in front of the fully grown bf16 GANSynth.train() at batch 8;
the feeds' own batches per second; gs_bank_gather against batch * length * 6 bytes at the HBM rate.  Results: profiles/bank_input.md.

The script generates its own notes (an examples.json index over 16-bit WAVs of 64000 random samples, all of them kept by the filter), so
it needs no dataset; the files have just been written when they are read: they are hot in the page cache, and cold files were not measured.

    python scripts/bench_input.py --mode feeds                     # batches per second of the two feeds, gs_bank_gather times
    python scripts/bench_input.py --mode train --feed host|bank|free [--root OTHER_CHECKOUT]

`--root` imports gansynth_amd from another checkout (built there): `--feed free --root <parent commit>` is the yardstick, taken on a tree
that has no bank at all.  One JSON line per result.
"""
import argparse
import json
import os
import sys
import tempfile
import time
import wave

import numpy as np

HBM_GBPS = 8000.0   # MI355X peak HBM rate (DESIGN.md's rooflines use the same figure)
LENGTH = 64000


def write_notes(directory, count, seed=0):
    """count WAVs of LENGTH random int16 samples under directory/audio and their examples.json; pitches cycle over 24..84, source 0."""
    rng = np.random.default_rng(seed)
    os.makedirs(os.path.join(directory, "audio"), exist_ok=True)
    index = {}
    for i in range(count):
        name = f"note_{i:05d}"
        with wave.open(os.path.join(directory, "audio", name + ".wav"), "wb") as w:
            w.setnchannels(1)
            w.setsampwidth(2)
            w.setframerate(16000)
            w.writeframes(rng.integers(-32768, 32768, size=LENGTH).astype("<i2").tobytes())
        index[name] = {"pitch": 24 + i % 61, "instrument_source": 0}
    path = os.path.join(directory, "examples.json")
    with open(path, "w") as f:
        json.dump(index, f)
    return path


def emit(obj):
    print(json.dumps(obj), flush=True)


def make_feed(kind, index, batch, torch, tmp):
    pitches = range(24, 85)
    if kind == "host":
        from gansynth_amd.dataset import nsynth_input_fn
        return nsynth_input_fn(index, batch, None, shuffle=True, pitches=pitches, sources=[0], device="cuda", seed=0)
    if kind == "bank":
        from gansynth_amd import bank
        path = os.path.join(tmp, "notes.bank")
        if not os.path.exists(path):
            bank.pack(index, path, pitches=pitches, sources=[0])
        return bank.bank_input_fn(path, batch, None, shuffle=True, pitches=pitches, sources=[0], device="cuda", seed=0)
    # free: sixteen batches of the same kind of data, on the device before the first iteration
    g = torch.Generator().manual_seed(0)
    pool = []
    for _ in range(16):
        wav = (torch.randint(-32768, 32768, (batch, LENGTH), generator=g).float() / 32768.0).cuda()
        lab = torch.nn.functional.one_hot(torch.randint(0, 61, (batch,), generator=g), 61).float().cuda()
        pool.append((wav, lab))
    at = [0]

    def free():
        at[0] += 1
        return pool[at[0] % len(pool)]

    free.finite = False
    return free


def feeds(args, torch, index, tmp):
    from gansynth_amd import kernels
    K = kernels.get()
    for kind, calls in (("host", args.host_batches), ("bank", args.bank_batches)):
        fn = make_feed(kind, index, args.batch, torch, tmp)
        for _ in range(8):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        emit({"feed": kind, "batch": args.batch, "batches": calls, "batches_per_second": calls / dt, "ms_per_batch": dt / calls * 1e3})
    # the launch alone: back to back on one stream between two events (at batch 8 the gap between launches is part of the figure)
    rows = 512
    pcm = torch.randint(-32768, 32768, (rows, LENGTH), dtype=torch.int16, device="cuda")
    classes = torch.randint(0, 61, (rows,), dtype=torch.int32, device="cuda")
    for batch in (8, 64):
        order = torch.randint(0, rows, (batch * 64,), dtype=torch.int32, device="cuda")
        for want_waves in (True, False):
            for i in range(16):
                K.bank_gather(pcm, classes, order, (i % 64) * batch, batch, 61, want_waves=want_waves)
            torch.cuda.synchronize()
            n = 512
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for i in range(n):
                K.bank_gather(pcm, classes, order, (i % 64) * batch, batch, 61, want_waves=want_waves)
            stop.record()
            torch.cuda.synchronize()
            us = start.elapsed_time(stop) / n * 1e3
            nbytes = batch * LENGTH * 6 if want_waves else batch * (8 + 61 * 4)
            emit({"kernel": "gs_bank_gather", "batch": batch, "waves": want_waves, "us_per_call": us, "bytes": nbytes,
                  "us_at_hbm_rate": nbytes / (HBM_GBPS * 1e3), "gb_per_second": nbytes / us / 1e3})


def train(args, torch, index, tmp):
    from gansynth_amd import variables
    from gansynth_amd.models import GANSynth
    from gansynth_amd.networks import PGGAN
    from gansynth_amd.utils import Dict
    torch.manual_seed(0)
    variables.set_default_store(variables.VariableStore(device="cuda", seed=0))
    pggan = PGGAN(min_resolution=[2, 16], max_resolution=[128, 1024], min_channels=32, max_channels=256, growing_level=1.0)
    feed = make_feed(args.feed, index, args.batch, torch, tmp)
    model = GANSynth(
        generator=pggan.generator, discriminator=pggan.discriminator, real_input_fn=feed,
        fake_input_fn=lambda: torch.randn(args.batch, 256, device="cuda"),
        spectral_params=Dict(waveform_length=LENGTH, sample_rate=16000, spectrogram_shape=[128, 1024], overlap=0.75),
        hyper_params=Dict(generator_learning_rate=8e-4, generator_beta1=0.0, generator_beta2=0.99, discriminator_learning_rate=8e-4,
                          discriminator_beta1=0.0, discriminator_beta2=0.99, mode_seeking_loss_weight=0.1, real_gradient_penalty_weight=5.0,
                          fake_gradient_penalty_weight=0.0),
        dtype=torch.bfloat16, use_graphs=True)
    done = 0
    windows = []
    for steps in [args.warmup] + [args.steps] * args.windows:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        done += steps
        model.train(None, None, total_steps=done, save_checkpoint_steps=0, log=None)   # (train() joins the pending update when it returns)
        torch.cuda.synchronize()
        windows.append((time.perf_counter() - t0) / steps * 1e3)
    assert model.global_step == done
    emit({"train": args.feed, "root": args.root, "batch": args.batch, "steps_per_window": args.steps, "warmup": args.warmup,
          "ms_per_iteration": [round(w, 4) for w in windows[1:]], "best_ms_per_iteration": min(windows[1:]),
          "generator_loss": float(model.generator_loss), "discriminator_loss": float(model.discriminator_loss)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["feeds", "train"], default="feeds")
    ap.add_argument("--feed", choices=["host", "bank", "free"], default="bank")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="the checkout gansynth_amd is imported from")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--notes", type=int, default=512)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--host_batches", type=int, default=300)
    ap.add_argument("--bank_batches", type=int, default=5000)
    args = ap.parse_args()
    args.root = os.path.abspath(args.root)
    sys.path.insert(0, args.root)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_input.py measures on the GPU: no device found")
    torch.cuda.set_device(0)
    with tempfile.TemporaryDirectory() as tmp:
        index = write_notes(tmp, args.notes) if (args.mode == "feeds" or args.feed != "free") else None
        (feeds if args.mode == "feeds" else train)(args, torch, index, tmp)


if __name__ == "__main__":
    main()
