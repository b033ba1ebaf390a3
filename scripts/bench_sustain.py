"""What holding notes past the waveform costs ("Sustain"): ONE gs_loop_search call and ONE gs_note_sustain call on waves of the
headline shape, and GANSynth.synthesize with and without held notes.

    python scripts/bench_sustain.py [--repeats 50] [--torch_repeats 3] [--synth_repeats 5] [--out profiles/sustain_bench.json]

Kernels: 200 notes x 64000 samples, every note held 8 s under a release of 1 s -- three pieces a note (64000, 16000 and 64000 samples),
600 rows behind the 200 generated ones -- under notes.sustain_plan(64000): 8001 lags of 2000 taps a note.  The two launches alternate
inside one loop (HIP events around each) after a warm-up; reported are the median, minimum and maximum of `--repeats` rounds in ms.
Next to each a torch restatement on the same device (the search: per note `unfold` of the span into [lags, W] and a matrix-vector
product, the energies by a cumulative sum; the waveform: per note an index computation and two gathers; `--torch_repeats` rounds), and
what bounds it: for the search 2 * lags * W FMAs a note (S_ab and S_bb) over the fp32 vector peak of the data sheet, for the waveform
the bytes it must move (4 * outputs written + 4 * distinct source samples read per piece) over the HBM rate measured here with a
device-to-device copy.
Score: scripts/bench_synthesize.py's score (200 notes over 60 s) with every fifth note held 8 s, through GANSynth.synthesize at the
headline model size with and without `sustain`, alternately; host seconds end to end and the device ms of the generator.
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

from scripts.bench_bend import hbm_rate           # noqa: E402
from scripts.bench_synthesize import make_score   # noqa: E402

NOTES, LENGTH, RATE = 200, 64000, 16000
HELD_SECONDS, RELEASE_SECONDS = 8.0, 1.0
PEAK_FP32_TFLOPS = 157.3     # MI355X data sheet: fp32 vector


def torch_search(x, a, m_min, m_max, window):
    """One note by torch: the span unfolded into [lags, W], a matrix-vector product, the energies by a cumulative sum."""
    w = x[a:a + window]
    span = x[a + m_min:a + m_max + window]
    s_ab = span.unfold(0, window, 1) @ w
    c = torch.cat([torch.zeros(1, device=x.device, dtype=torch.float64), (span.double() ** 2).cumsum(0)])
    s_bb = (c[window:] - c[:-window]).float()
    prod = (w * w).sum() * s_bb
    return torch.where(prod == 0, torch.zeros_like(prod), s_ab / prod.sqrt())


def torch_sustain(x, a, m, xfade, offset, count):
    """One piece by torch: the indices, two gathers, the crossfade."""
    k = offset + torch.arange(count, device=x.device)
    b = a + m
    p = torch.where(k >= b, (k - b) % m, torch.zeros_like(k))
    w = (p + 1).float() * (1.0 / (xfade + 1))
    fade = p < xfade
    looped = torch.where(fade, (1 - w) * x[torch.where(fade, b + p, torch.zeros_like(p))] + w * x[a + p], x[a + p])
    return torch.where(k < b, x[k.clamp(max=b - 1)], looped)


def events():
    return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def stats(ms):
    ms = sorted(ms)
    return dict(median=ms[len(ms) // 2], min=ms[0], max=ms[-1])


def measure_kernels(repeats, torch_repeats):
    from gansynth_amd import _lib, kernels, notes as N
    K = kernels.get()
    a, m_min, m_max, window, xfade = plan = N.sustain_plan(LENGTH)
    n_lags = m_max - m_min + 1
    pieces = N.sustain_pieces(int(HELD_SECONDS * RATE), int(RELEASE_SECONDS * RATE), LENGTH)
    rows = NOTES * (1 + len(pieces))
    waves = torch.empty(rows, LENGTH, device="cuda")
    # decaying harmonic tones with a little noise, a period per note: what a loop search is for
    n = torch.arange(LENGTH, device="cuda", dtype=torch.float64)
    periods = np.random.default_rng(0).uniform(30.0, 400.0, NOTES)
    for i, period in enumerate(periods):
        tone = sum(torch.sin(2 * np.pi * h * n / period) / h for h in range(1, 6)) * torch.exp(-n / (2.0 * LENGTH))
        waves[i] = (0.3 * tone).float() + 1e-3 * torch.randn(LENGTH, device="cuda")

    def upload(arr):
        return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).cuda()

    search_table = upload(kernels.loop_search_table([(i, a, m_min, m_max, window) for i in range(NOTES)], rows, LENGTH, n_lags))
    scores = torch.empty(NOTES, n_lags, device="cuda")

    def search():
        _lib.check(K.lib.gs_loop_search(waves.data_ptr(), rows, LENGTH, LENGTH, search_table.data_ptr(), NOTES, scores.data_ptr(), n_lags,
                                        kernels._stream()), "gs_loop_search")

    search()
    t0 = time.perf_counter()
    host_scores = scores.cpu().numpy()
    picks = [N.pick_loop(host_scores[i], m_min) for i in range(NOTES)]
    pick_seconds = time.perf_counter() - t0
    jobs = [(i, NOTES + i * len(pieces) + j, offset, hold + release, a, picks[i], xfade)
            for i in range(NOTES) for j, (offset, hold, release) in enumerate(pieces)]
    job_table = upload(kernels.note_sustain_table(jobs, rows, LENGTH))

    def sustain():
        _lib.check(K.lib.gs_note_sustain(waves.data_ptr(), rows, LENGTH, LENGTH, job_table.data_ptr(), len(jobs), kernels._stream()), "gs_note_sustain")

    runs = {"loop_search": search, "note_sustain": sustain}
    for _ in range(5):
        for run in runs.values():
            run()
    pairs = {name: [] for name in runs}
    for _ in range(repeats):
        for name, run in runs.items():
            e0, e1 = events()
            e0.record()
            run()
            e1.record()
            pairs[name].append((e0, e1))
    torch.cuda.synchronize()
    rate = hbm_rate()
    ms = {name: stats([x.elapsed_time(y) for x, y in pairs[name]]) for name in runs}

    # torch, per note, on the same device; its results against the kernels'
    torch_ms = {name: [] for name in runs}
    worst = dict.fromkeys(runs, 0.0)
    for i in range(1 + torch_repeats):
        e0, e1 = events()
        e0.record()
        for r in range(NOTES):
            s = torch_search(waves[r], a, m_min, m_max, window)
            if i == 0:
                worst["loop_search"] = max(worst["loop_search"], float((s - scores[r]).abs().max()))
        e1.record()
        torch.cuda.synchronize()
        f0, f1 = events()
        f0.record()
        for src, dst, offset, count, _, m, _ in jobs:
            y = torch_sustain(waves[src], a, m, xfade, offset, count)
            if i == 0:
                worst["note_sustain"] = max(worst["note_sustain"], float((y - waves[dst, :count]).abs().max()))
        f1.record()
        torch.cuda.synchronize()
        if i:
            torch_ms["loop_search"].append(e0.elapsed_time(e1))
            torch_ms["note_sustain"].append(f0.elapsed_time(f1))

    fmas = 2.0 * NOTES * n_lags * window
    outputs = sum(job[3] for job in jobs)
    distinct = 0
    for _, _, offset, count, _, m, _ in jobs:
        k = offset + np.arange(count, dtype=np.int64)
        b = a + m
        p = (k - b) % m
        seen = np.zeros(LENGTH, dtype=bool)
        seen[np.concatenate([k[k < b], (a + p)[k >= b], (b + p)[(k >= b) & (p < xfade)]])] = True
        distinct += int(seen.sum())
    nbytes = 4 * (outputs + distinct)
    out = {}
    for name in runs:
        t = stats(torch_ms[name])
        out[name] = dict(ms=ms[name], torch_ms=t, torch_over_kernel=t["median"] / ms[name]["median"], torch_max_difference=worst[name])
    out["loop_search"].update(lags=n_lags, window=window, fmas=fmas, fma_roof_ms=fmas / (PEAK_FP32_TFLOPS / 2 * 1e12) * 1e3,
                              gfma_per_s=fmas / ms["loop_search"]["median"] / 1e6,
                              share_of_fp32_peak=fmas / (PEAK_FP32_TFLOPS / 2 * 1e12) * 1e3 / ms["loop_search"]["median"])
    out["note_sustain"].update(jobs=len(jobs), outputs=outputs, bytes=nbytes, hbm_roof_ms=nbytes / rate / 1e6,
                               gb_per_s=nbytes / ms["note_sustain"]["median"] / 1e6,
                               share_of_copy_rate=nbytes / rate / 1e6 / ms["note_sustain"]["median"])
    return dict(notes=NOTES, length=LENGTH, plan=list(plan), pieces=[list(p) for p in pieces], hbm_gb_per_s=rate, host_pick_seconds=pick_seconds,
                loops=dict(min=min(picks), max=max(picks)), **out)


def measure_score(repeats, batch=8):
    from gansynth_amd import variables
    from gansynth_amd.models import GANSynth
    from gansynth_amd.networks import PGGAN
    from gansynth_amd.notes import Note
    from gansynth_amd.utils import Dict
    variables.set_default_store(variables.VariableStore(device="cuda", seed=0))
    pggan = PGGAN(min_resolution=[2, 16], max_resolution=[128, 1024], min_channels=32, max_channels=256, growing_level=1.0)
    spectral = Dict(waveform_length=LENGTH, sample_rate=RATE, spectrogram_shape=[128, 1024], overlap=0.75)
    model = GANSynth(pggan.generator, pggan.discriminator, None, None, spectral, Dict(), dtype=torch.bfloat16)
    notes = [Note(n.pitch, n.velocity, n.start, n.start + HELD_SECONDS) if i % 5 == 0 else n for i, n in enumerate(make_score(200, 60.0))]
    model._build(torch.zeros(batch, 256, device="cuda", dtype=torch.bfloat16), torch.zeros(batch, 61, device="cuda", dtype=torch.bfloat16))
    timed_events = []
    generator = model.generator

    def timed(*a, **kw):
        e0, e1 = events()
        e0.record()
        out = generator(*a, **kw)
        e1.record()
        timed_events.append((e0, e1))
        return out

    model.generator = timed
    calls = {"cut": [], "held": []}
    infos = {}
    for i in range(1 + repeats):
        for which, how in (("cut", dict()), ("held", dict(sustain=True))):
            timed_events.clear()
            infos[which] = info = {}
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            model.synthesize(notes, want_pcm=True, info=info, batch_size=batch, **how)
            torch.cuda.synchronize()
            seconds = time.perf_counter() - t0
            if i:
                calls[which].append(dict(seconds=seconds, generator_ms=sum(a.elapsed_time(b) for a, b in timed_events), chunks=len(timed_events)))
    out = {}
    for which, rows in calls.items():
        s = sorted(r["seconds"] for r in rows)
        out[which] = dict(seconds=dict(median=s[len(s) // 2], min=s[0], max=s[-1]), generator_ms_per_chunk=rows[0]["generator_ms"] / rows[0]["chunks"],
                          chunks=rows[0]["chunks"], total_samples=infos[which]["total_samples"])
    held = infos["held"]
    return dict(notes=len(held["notes"]), held_notes=held["held_notes"], sustain_rows=held["sustain_rows"], repeats=repeats, **out,
                sustain_adds_seconds=out["held"]["seconds"]["median"] - out["cut"]["seconds"]["median"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--torch_repeats", type=int, default=3)
    ap.add_argument("--synth_repeats", type=int, default=5)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sustain.py measures on the GPU: no device found")
    torch.cuda.set_device(0)
    result = dict(config=dict(repeats=args.repeats, torch_repeats=args.torch_repeats, sample_rate=RATE, held_seconds=HELD_SECONDS,
                              release_seconds=RELEASE_SECONDS, peak_fp32_tflops=PEAK_FP32_TFLOPS),
                  kernels=measure_kernels(args.repeats, args.torch_repeats), score=measure_score(args.synth_repeats))
    print(json.dumps(result))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
