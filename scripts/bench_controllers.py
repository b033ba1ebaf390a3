"""What controller curves cost ("Controllers"): ONE gs_note_mix_curves call next to ONE gs_note_mix_stereo call on the same notes.

    python scripts/bench_controllers.py [--repeats 50] [--out FILE]

The two scores of scripts/bench_ensemble.py (sparse: 200 notes over 60 s; dense: 3000 notes over 200 s) on waves of the headline shape, every
note in one of 8 parts (note n in part n % 8, so that neighbouring candidates change part).  Three forms, each normalising and writing PCM:
  stereo     gs_note_mix_stereo with gain_l = gain_r = gain
  constant   gs_note_mix_curves, every part's curve the one point (0, 1, 1) -- bit for bit the stereo mix, which is checked before timing
  ramps      gs_note_mix_curves, every part's curve a breakpoint every 10 ms (160 samples) over the whole clip
The forms alternate inside one loop (HIP events around each) after a warm-up of all three; reported are the median, minimum and maximum
of `--repeats` rounds in ms and the ratio of each curve form's median to the stereo mix's.  Needs a GPU; prints one JSON object.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from scripts.bench_ensemble import LENGTH, RATE, make_score   # noqa: E402

PARTS, STEP = 8, 160


def measure(name, count, seconds, repeats):
    from gansynth_amd import _lib, kernels, notes as N
    K = kernels.get()
    score = make_score(count, seconds)
    kept, table, total, _ = N.schedule(score, range(24, 85), RATE, LENGTH, 1.0)
    waves = (torch.rand(len(kept), LENGTH, device="cuda") * 2 - 1) * 0.3

    def upload(arr):
        return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).cuda()

    stereo_table = upload(kernels.note_mix_stereo_table([row + (row[4],) for row in table], len(kept), LENGTH, total))
    curve_rows = [row + (n % PARTS,) for n, row in enumerate(table)]
    rng = np.random.default_rng(2)
    positions = list(range(0, total, STEP))
    forms = {"constant": ([(0, 1.0, 1.0)] * PARTS, list(range(PARTS + 1))),
             "ramps": ([(pos, float(l), float(r)) for _ in range(PARTS) for pos, (l, r) in zip(positions, rng.random((len(positions), 2)))],
                       [p * len(positions) for p in range(PARTS + 1)])}
    tables = {form: [upload(a) for a in kernels.note_mix_curves_table(curve_rows, points, first, len(kept), LENGTH, total)]
              for form, (points, first) in forms.items()}
    stride = (total + 3) // 4 * 4
    out = torch.empty((2, stride), dtype=torch.float32, device="cuda")
    other = torch.empty((2, stride), dtype=torch.float32, device="cuda")
    pcm = torch.empty((total, 2), dtype=torch.int16, device="cuda")
    peak = torch.empty(2, dtype=torch.float32, device="cuda")
    ws = torch.empty(max(K.lib.gs_note_mix_curves_workspace_bytes(total), 256), dtype=torch.uint8, device="cuda")

    def stereo(normalize=1, dst=out):
        _lib.check(K.lib.gs_note_mix_stereo(waves.data_ptr(), len(kept), LENGTH, LENGTH, stereo_table.data_ptr(), len(kept), total, normalize,
                                            dst.data_ptr(), stride, pcm.data_ptr(), peak.data_ptr(), ws.data_ptr(), ws.numel(), kernels._stream()),
                   "gs_note_mix_stereo")

    def curves(form, normalize=1, dst=out):
        notes, points, first = tables[form]
        _lib.check(K.lib.gs_note_mix_curves(waves.data_ptr(), len(kept), LENGTH, LENGTH, notes.data_ptr(), len(kept), points.data_ptr(),
                                            len(forms[form][0]), first.data_ptr(), PARTS, 2, total, normalize, dst.data_ptr(), stride, pcm.data_ptr(),
                                            peak[1:].data_ptr(), ws.data_ptr(), ws.numel(), kernels._stream()), "gs_note_mix_curves")

    stereo(0, out)
    curves("constant", 0, other)
    torch.cuda.synchronize()
    if not (torch.equal(out[:, :total], other[:, :total]) and float(peak[0]) == float(peak[1])):
        raise SystemExit(f"{name}: constant curves of 1 do not give the stereo mix")
    runs = {"stereo": stereo, "constant": lambda: curves("constant"), "ramps": lambda: curves("ramps")}
    for _ in range(5):
        for fn in runs.values():
            fn()
    pairs = {which: [] for which in runs}
    for _ in range(repeats):
        for which, fn in runs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            pairs[which].append((e0, e1))
    torch.cuda.synchronize()
    ms = {which: sorted(a.elapsed_time(b) for a, b in p) for which, p in pairs.items()}
    stats = {which: dict(median=v[len(v) // 2], min=v[0], max=v[-1]) for which, v in ms.items()}
    spans = np.array([min(h + r, total - o) for o, h, r, _, _ in table], dtype=np.int64)
    return dict(notes=len(kept), parts=PARTS, clip_seconds=total / RATE, mean_overlap=float(spans.sum()) / total,
                points=dict(constant=PARTS, ramps=PARTS * len(positions)), stereo_ms=stats["stereo"], constant_ms=stats["constant"],
                ramps_ms=stats["ramps"], constant_over_stereo=stats["constant"]["median"] / stats["stereo"]["median"],
                ramps_over_stereo=stats["ramps"]["median"] / stats["stereo"]["median"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_controllers.py measures on the GPU: no device found")
    torch.cuda.set_device(0)
    result = dict(config=dict(length=LENGTH, sample_rate=RATE, repeats=args.repeats, normalize=True, pcm=True, breakpoint_samples=STEP),
                  sparse=measure("sparse", 200, 60.0, args.repeats), dense=measure("dense", 3000, 200.0, args.repeats))
    print(json.dumps(result))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
