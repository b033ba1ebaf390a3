"""What pitch bend costs ("Pitch bend"): ONE gs_note_warp call on waves of the headline shape, and GANSynth.synthesize with
and without bent notes.

    python scripts/bench_bend.py [--repeats 50] [--torch_repeats 3] [--synth_repeats 5] [--out profiles/bend_bench.json]

Kernel: 200 notes x 64000 samples, every note bent over its whole length, under four curves --
  one        the constant ratio 1 (every coefficient but one an exact 0: the cost of the pass itself, 64 taps)
  tone       the constant ratio 2^(2/12) (72 taps)
  four       the constant ratio 4 (256 taps, the widest filter; three quarters of every row are zeros past the waveform's end)
  vibrato    a 6 Hz wheel vibrato of half a semitone either way, a point every 160 samples over the clip
-- alternating inside one loop (HIP events around each) after a warm-up of all four; reported are the median, minimum and maximum of
`--repeats` rounds in ms.  Next to each: a torch restatement on the same device (per note: gather the taps, evaluate the coefficients
from the table, multiply and sum; positions precomputed, `--torch_repeats` rounds) and the two roofs -- the bytes the pass must move
(4 * source samples it can reach + 4 * count per note) over the HBM rate measured here with a device-to-device copy, and count * taps
FMAs over the fp32 vector peak of the data sheet.
Score: scripts/bench_synthesize.py's score (200 notes over 60 s) in five parts, part 0 -- a fifth of the notes -- under the vibrato,
through GANSynth.synthesize at the headline model size with and without `bend`, alternately; host seconds end to end and the device ms
of the generator.  Needs a GPU; prints one JSON object.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from scripts.bench_synthesize import make_score   # noqa: E402

NOTES, LENGTH, RATE, STEP = 200, 64000, 16000, 160
Z, Q = 32, 256
PEAK_FP32_TFLOPS = 157.3     # MI355X data sheet: fp32 vector


def with_cum(rows):
    out = []
    for i, (pos, ratio) in enumerate(rows):
        if i == 0:
            cum = ratio * float(pos)
        else:
            p0, r0, c0 = out[-1]
            d = float(pos) - p0
            cum = c0 + r0 * d + (ratio - r0) * d * d / (2.0 * d)
        out.append((float(pos), float(ratio), cum))
    return out


def vibrato(total):
    t = np.arange(0, total + STEP, STEP)
    return with_cum(list(zip(t.tolist(), (2.0 ** (0.5 * np.sin(2 * np.pi * 6.0 * t / RATE) / 12)).tolist())))


def positions(points, onset, count):
    """(n, f, c) of a note under one curve, float64 on the host (the rule of DESIGN.md "Pitch bend")."""
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    pos, ratio, cum = pts[:, 0], pts[:, 1], pts[:, 2]

    def phi(t):
        k = np.searchsorted(pos, t, side="right")
        i0, i1 = np.maximum(k - 1, 0), np.minimum(k, len(pos) - 1)
        d, dp = t - pos[i0], pos[i1] - pos[i0]
        flat = (i0 == i1) | (k == 0)
        safe = np.where(flat, 1.0, dp)
        dr = np.where(flat, 0.0, ratio[i1] - ratio[i0])
        return cum[i0] + ratio[i0] * d + dr * d * d / (2.0 * safe), ratio[i0] + dr * d / safe

    p, r = phi(float(onset) + np.arange(count, dtype=np.float64))
    q = p - phi(np.array([float(onset)]))[0][0]
    n = np.floor(q)
    return n.astype(np.int64), (q - n).astype(np.float32), np.minimum(1.0, 1.0 / r).astype(np.float32)


def torch_warp(x, table, n, f, c, half):
    """One note by torch: taps j in [-half + 1, half] gathered from the zero-padded row, coefficients from the table, product, sum."""
    j = torch.arange(-half + 1, half + 1, device=x.device)
    idx = n[:, None] + j[None]
    inside = (idx >= 0) & (idx < x.numel())
    xs = torch.where(inside, x[idx.clamp(0, x.numel() - 1)], torch.zeros((), device=x.device))
    a = torch.clamp(c[:, None] * (j[None].float() - f[:, None]).abs() * Q, max=float(Z * Q))
    m = a.long()
    t0 = table[m]
    h = c[:, None] * (t0 + (a - m.float()) * (table[m + 1] - t0))
    return (h * xs).sum(dim=1)


def hbm_rate():
    a = torch.empty(1 << 28, dtype=torch.uint8, device="cuda")
    b = torch.empty_like(a)
    for _ in range(3):
        b.copy_(a)
    pairs = []
    for _ in range(20):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        b.copy_(a)
        e1.record()
        pairs.append((e0, e1))
    torch.cuda.synchronize()
    ms = sorted(x.elapsed_time(y) for x, y in pairs)
    return 2 * a.numel() / ms[len(ms) // 2] / 1e6      # GB/s, read + written


def measure_kernel(repeats, torch_repeats):
    from gansynth_amd import _lib, kernels
    K = kernels.get()
    rng = np.random.default_rng(0)
    onsets = np.sort(rng.integers(0, 55 * RATE, NOTES)).tolist()
    total = max(onsets) + LENGTH
    waves = torch.empty(2 * NOTES, LENGTH, device="cuda")
    waves[:NOTES] = (torch.rand(NOTES, LENGTH, device="cuda") * 2 - 1) * 0.3
    notes = [(n, NOTES + n, onsets[n], LENGTH, 0) for n in range(NOTES)]
    forms = {"one": with_cum([(0, 1.0)]), "tone": with_cum([(0, 2.0 ** (2 / 12))]), "four": with_cum([(0, 4.0)]), "vibrato": vibrato(total)}
    table = K.note_warp_table_dev("cuda")

    def upload(arr):
        return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).cuda()

    tables = {form: [upload(a) for a in kernels.note_warp_table(notes, points, [0, len(points)], 2 * NOTES, LENGTH)] for form, points in forms.items()}

    def run(form):
        nts, pts, first = tables[form]
        _lib.check(K.lib.gs_note_warp(waves.data_ptr(), 2 * NOTES, LENGTH, LENGTH, nts.data_ptr(), NOTES, pts.data_ptr(), first.data_ptr(), 1,
                                      len(forms[form]), table.data_ptr(), kernels._stream()), "gs_note_warp")

    for _ in range(5):
        for form in forms:
            run(form)
    pairs = {form: [] for form in forms}
    for _ in range(repeats):
        for form in forms:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(form)
            e1.record()
            pairs[form].append((e0, e1))
    torch.cuda.synchronize()
    rate = hbm_rate()
    out = {}
    for form, points in forms.items():
        ms = sorted(a.elapsed_time(b) for a, b in pairs[form])
        where = [positions(points, onsets[n], LENGTH) for n in range(NOTES)]
        taps = float(sum((2 * np.ceil(Z / c.astype(np.float64))).sum() for _, _, c in where))
        reach = sum(min(LENGTH, int(n[-1]) + 1) for n, _, _ in where)
        nbytes = 4 * reach + 4 * LENGTH * NOTES
        # torch, per note, on the positions above; its result against the kernel's on the last note
        dev = [(torch.from_numpy(n).cuda(), torch.from_numpy(f).cuda(), torch.from_numpy(c).cuda()) for n, f, c in where]
        half = int(max(np.ceil(Z / c.min()) for _, _, c in where))
        run(form)
        tms = []
        for i in range(1 + torch_repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for n in range(NOTES):
                y = torch_warp(waves[n], table, *dev[n], half)
            e1.record()
            torch.cuda.synchronize()
            if i:
                tms.append(e0.elapsed_time(e1))
        scale = float(waves[NOTES - 1].abs().max()) + 1e-30
        agree = float((y - waves[2 * NOTES - 1]).abs().max()) / scale
        tms.sort()
        median = ms[len(ms) // 2]
        out[form] = dict(ms=dict(median=median, min=ms[0], max=ms[-1]), points=len(points), taps_per_output=taps / (NOTES * LENGTH),
                         torch_ms=dict(median=tms[len(tms) // 2], min=tms[0], max=tms[-1]), torch_over_kernel=tms[len(tms) // 2] / median,
                         torch_max_difference=agree, bytes=nbytes, hbm_roof_ms=nbytes / rate / 1e6,
                         fma_roof_ms=taps / (PEAK_FP32_TFLOPS / 2 * 1e12) * 1e3, gtaps_per_s=taps / median / 1e6)
    return dict(notes=NOTES, length=LENGTH, hbm_gb_per_s=rate, forms=out)


def measure_score(repeats, batch=8):
    from gansynth_amd import notes as N, variables
    from gansynth_amd.models import GANSynth
    from gansynth_amd.networks import PGGAN
    from gansynth_amd.utils import Dict
    variables.set_default_store(variables.VariableStore(device="cuda", seed=0))
    pggan = PGGAN(min_resolution=[2, 16], max_resolution=[128, 1024], min_channels=32, max_channels=256, growing_level=1.0)
    spectral = Dict(waveform_length=LENGTH, sample_rate=RATE, spectrogram_shape=[128, 1024], overlap=0.75)
    model = GANSynth(pggan.generator, pggan.discriminator, None, None, spectral, Dict(), dtype=torch.bfloat16)
    notes = make_score(200, 60.0)
    score = N.Score(notes, [n % 5 for n in range(len(notes))], [N.DEFAULT_VOLUME] * len(notes), [None] * len(notes), [N.Part(None, None)] * 5)
    wheel = [(s / RATE, 0.5 * float(np.sin(2 * np.pi * 6.0 * s / RATE))) for s in range(0, 66 * RATE, STEP)]
    bends = [wheel, [], [], [], []]
    model._build(torch.zeros(batch, 256, device="cuda", dtype=torch.bfloat16), torch.zeros(batch, 61, device="cuda", dtype=torch.bfloat16))
    events = []
    generator = model.generator

    def timed(*a, **kw):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = generator(*a, **kw)
        e1.record()
        events.append((e0, e1))
        return out

    model.generator = timed
    calls = {"plain": [], "bent": []}
    info = {}
    for i in range(1 + repeats):
        for which, what, how in (("plain", notes, dict()), ("bent", score, dict(bend=bends, controller_ramp=0.01))):
            events.clear()
            info = {}
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            model.synthesize(what, want_pcm=True, info=info, batch_size=batch, **how)
            torch.cuda.synchronize()
            seconds = time.perf_counter() - t0
            if i:
                calls[which].append(dict(seconds=seconds, generator_ms=sum(a.elapsed_time(b) for a, b in events), chunks=len(events)))
    stats = {}
    for which, rows in calls.items():
        s = sorted(r["seconds"] for r in rows)
        stats[which] = dict(seconds=dict(median=s[len(s) // 2], min=s[0], max=s[-1]), generator_ms_per_chunk=rows[0]["generator_ms"] / rows[0]["chunks"],
                            chunks=rows[0]["chunks"])
    return dict(notes=len(info["notes"]), bent_notes=info["bent_notes"], bend_points=info["bend_points"], repeats=repeats, **stats,
                bend_adds_seconds=stats["bent"]["seconds"]["median"] - stats["plain"]["seconds"]["median"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--torch_repeats", type=int, default=3)
    ap.add_argument("--synth_repeats", type=int, default=5)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_bend.py measures on the GPU: no device found")
    torch.cuda.set_device(0)
    result = dict(config=dict(repeats=args.repeats, torch_repeats=args.torch_repeats, sample_rate=RATE, breakpoint_samples=STEP,
                              peak_fp32_tflops=PEAK_FP32_TFLOPS),
                  kernel=measure_kernel(args.repeats, args.torch_repeats), score=measure_score(args.synth_repeats))
    print(json.dumps(result))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
