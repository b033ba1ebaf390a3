"""What rendering a score costs ("Note sequences").

    python scripts/bench_synthesize.py [--notes 200] [--seconds 60] [--repeats 5] [--mix_repeats 50] [--output_rate HZ] [--out FILE]

A fixed generated score -- `--notes` notes over `--seconds` seconds, seeded, built here -- through GANSynth.synthesize at the headline
model size (fully grown 128 x 1024 generator, batch 8, bf16, initial weights: the cost does not depend on them).  One warm-up call, then
`--repeats` timed ones.  Reported, per call: device ms of the generator chunks and of the inverse transform (HIP events around each),
device ms of gs_note_mix alone (HIP events around `--mix_repeats` calls of the entry point on the call's own waves and table, with
normalisation and PCM), notes per second end to end (host clock around synthesize, which ends in a device synchronise: info's peak is
read), and the mix's algorithmic bytes -- 4 * sum(hold + release) read, 4 * T written, + 2 * T with pcm -- over its time.
`--output_rate HZ`: the clip is rendered at that rate (synthesize's sample_rate: the mix unnormalised, then one gs_resample call with
the normalisation and the PCM); the difference of `seconds_end_to_end` to a run without the flag is what the rate change adds.
Needs a GPU; prints one JSON object.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make_score(count, seconds, seed=0):
    from gansynth_amd.notes import Note
    rng = np.random.default_rng(seed)
    starts = np.sort(rng.random(count) * (seconds - 5.0))
    lengths = np.exp(rng.uniform(np.log(0.1), np.log(4.0), count))
    return [Note(int(p), int(v), float(s), float(s + d)) for p, v, s, d in zip(rng.integers(24, 85, count), rng.integers(30, 128, count), starts, lengths)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--notes", type=int, default=200)
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--mix_repeats", type=int, default=50)
    ap.add_argument("--output_rate", type=int, default=None)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_synthesize.py measures on the GPU: no device found")

    from gansynth_amd import _lib, kernels, notes as N, spectral_ops, variables
    from gansynth_amd.models import GANSynth
    from gansynth_amd.networks import PGGAN
    from gansynth_amd.utils import Dict

    torch.cuda.set_device(0)
    variables.set_default_store(variables.VariableStore(device="cuda", seed=0))
    pggan = PGGAN(min_resolution=[2, 16], max_resolution=[128, 1024], min_channels=32, max_channels=256, growing_level=1.0)
    spectral = Dict(waveform_length=64000, sample_rate=16000, spectrogram_shape=[128, 1024], overlap=0.75)
    model = GANSynth(pggan.generator, pggan.discriminator, None, None, spectral, Dict(), dtype=torch.bfloat16)
    score = make_score(args.notes, args.seconds)
    model._build(torch.zeros(args.batch, 256, device="cuda", dtype=torch.bfloat16), torch.zeros(args.batch, 61, device="cuda", dtype=torch.bfloat16))

    events = {"generator": [], "inverse": []}

    def timed(which, fn):
        def wrapper(*a, **kw):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn(*a, **kw)
            e1.record()
            events[which].append((e0, e1))
            return out
        return wrapper

    model.generator = timed("generator", model.generator)
    inverse = spectral_ops.convert_images_to_waveform
    spectral_ops.convert_images_to_waveform = timed("inverse", inverse)
    calls = []
    try:
        for i in range(1 + args.repeats):
            for v in events.values():
                v.clear()
            info = {}
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            model.synthesize(score, want_pcm=True, info=info, batch_size=args.batch, sample_rate=args.output_rate)
            torch.cuda.synchronize()
            seconds = time.perf_counter() - t0
            if i:   # (the first call builds the variables, prepares the weights and plans the inverse transform)
                calls.append(dict(seconds=seconds, generator_ms=sum(a.elapsed_time(b) for a, b in events["generator"]),
                                  inverse_ms=sum(a.elapsed_time(b) for a, b in events["inverse"]), chunks=len(events["generator"])))
    finally:
        spectral_ops.convert_images_to_waveform = inverse

    # gs_note_mix alone, on the same table and on waves of the same shape
    K = kernels.get()
    kept, table, total, dropped = N.schedule(score, range(24, 85), 16000, 64000, 1.0)
    waves = (torch.rand(len(kept), 64000, device="cuda") * 2 - 1) * 0.3
    arr = kernels.note_mix_table(table, len(kept), 64000, total)
    dev_table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).cuda()
    out = torch.empty(total, dtype=torch.float32, device="cuda")
    pcm = torch.empty(total, dtype=torch.int16, device="cuda")
    peak = torch.empty(1, dtype=torch.float32, device="cuda")
    ws = torch.empty(max(K.lib.gs_note_mix_workspace_bytes(total), 256), dtype=torch.uint8, device="cuda")

    def mix():
        _lib.check(K.lib.gs_note_mix(waves.data_ptr(), len(kept), 64000, 64000, dev_table.data_ptr(), len(arr), total, 1, out.data_ptr(),
                                     pcm.data_ptr(), peak.data_ptr(), ws.data_ptr(), ws.numel(), kernels._stream()), "gs_note_mix")

    for _ in range(5):
        mix()
    pairs = []
    for _ in range(args.mix_repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        mix()
        e1.record()
        pairs.append((e0, e1))
    torch.cuda.synchronize()
    mix_ms = sorted(a.elapsed_time(b) for a, b in pairs)
    read = 4 * sum(min(h + r, total - o) for o, h, r, _, _ in table)
    written = 4 * total + 2 * total
    median = mix_ms[len(mix_ms) // 2]
    best = min(calls, key=lambda c: c["seconds"])
    result = dict(config=dict(notes=len(kept), dropped=dropped, clip_seconds=total / 16000, batch=args.batch, dtype="bf16", resolution=[128, 1024],
                              repeats=args.repeats, mix_repeats=args.mix_repeats, output_rate=args.output_rate or 16000),
                  calls=calls, generator_ms=best["generator_ms"], inverse_ms=best["inverse_ms"], seconds_end_to_end=best["seconds"],
                  notes_per_second=len(kept) / best["seconds"],
                  note_mix_ms=dict(median=median, min=mix_ms[0], max=mix_ms[-1]),
                  note_mix_bytes=dict(read=read, written=written), note_mix_gb_per_s=(read + written) / median / 1e6, peak=info["peak"])
    print(json.dumps(result))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
