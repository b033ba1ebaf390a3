"""What two channels cost ("Parts and stereo"): ONE gs_note_mix_stereo call next to what two channels took before it, TWO
gs_note_mix calls with the left and the right gains.

    python scripts/bench_ensemble.py [--repeats 50] [--out FILE]

Two generated scores, seeded, built here, on waves of the headline shape (64000 samples a note):
  sparse   bench_synthesize.py's score: 200 notes over 60 s, about 8 sounding at once
  dense    3000 notes over 200 s, about 30 sounding at once
Each call normalises and writes PCM.  The two forms alternate inside one loop (HIP events around each), after a warm-up of both; reported
are the median, minimum and maximum of `--repeats` rounds, and for the fused call its algorithmic bytes -- 4 * sum(hold + release) read
once, 2 * 4 * T of fp32 and 2 * 2 * T of PCM written -- over its median time.  The mixes themselves are compared before anything is timed:
each channel of the fused call, unnormalised, must equal the mono call's bit for bit.
Needs a GPU; prints one JSON object.
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LENGTH, RATE = 64000, 16000


def make_score(count, seconds, seed=0):
    """bench_synthesize.py's draw: starts uniform over the clip, lengths log-uniform in 0.1 .. 4 s."""
    from gansynth_amd.notes import Note
    rng = np.random.default_rng(seed)
    starts = np.sort(rng.random(count) * (seconds - 5.0))
    lengths = np.exp(rng.uniform(np.log(0.1), np.log(4.0), count))
    return [Note(int(p), int(v), float(s), float(s + d)) for p, v, s, d in zip(rng.integers(24, 85, count), rng.integers(30, 128, count), starts, lengths)]


def measure(name, count, seconds, repeats):
    from gansynth_amd import _lib, kernels, notes as N
    K = kernels.get()
    score = make_score(count, seconds)
    kept, table, total, _ = N.schedule(score, range(24, 85), RATE, LENGTH, 1.0)
    rng = np.random.default_rng(1)
    pans = rng.uniform(-1.0, 1.0, len(kept))
    stereo = [row[:4] + (float(np.float32(row[4] * math.cos((p + 1) * math.pi / 4))), float(np.float32(row[4] * math.sin((p + 1) * math.pi / 4))))
              for row, p in zip(table, pans)]
    waves = (torch.rand(len(kept), LENGTH, device="cuda") * 2 - 1) * 0.3

    def upload(arr):
        return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).cuda()

    fused_table = upload(kernels.note_mix_stereo_table(stereo, len(kept), LENGTH, total))
    side_tables = [upload(kernels.note_mix_table([row[:4] + (row[4 + c],) for row in stereo], len(kept), LENGTH, total)) for c in (0, 1)]
    stride = (total + 3) // 4 * 4
    out = torch.empty((2, stride), dtype=torch.float32, device="cuda")
    pcm = torch.empty((total, 2), dtype=torch.int16, device="cuda")
    sides = torch.empty((2, stride), dtype=torch.float32, device="cuda")
    side_pcm = torch.empty((2, stride), dtype=torch.int16, device="cuda")   # (both rows on 8 bytes: the mono finish stays on its wide path)
    peak = torch.empty(3, dtype=torch.float32, device="cuda")
    ws = torch.empty(max(K.lib.gs_note_mix_stereo_workspace_bytes(total), 256), dtype=torch.uint8, device="cuda")

    def fused(normalize=1):
        _lib.check(K.lib.gs_note_mix_stereo(waves.data_ptr(), len(kept), LENGTH, LENGTH, fused_table.data_ptr(), len(kept), total, normalize,
                                            out.data_ptr(), stride, pcm.data_ptr(), peak.data_ptr(), ws.data_ptr(), ws.numel(), kernels._stream()),
                   "gs_note_mix_stereo")

    def two_mono(normalize=1):
        for c in (0, 1):
            _lib.check(K.lib.gs_note_mix(waves.data_ptr(), len(kept), LENGTH, LENGTH, side_tables[c].data_ptr(), len(kept), total, normalize,
                                         sides[c].data_ptr(), side_pcm[c].data_ptr(), peak[1 + c:].data_ptr(), ws.data_ptr(), ws.numel(),
                                         kernels._stream()), "gs_note_mix")

    fused(0)
    two_mono(0)
    torch.cuda.synchronize()
    if not (torch.equal(out[:, :total], sides[:, :total]) and float(peak[0]) == max(float(peak[1]), float(peak[2]))):
        raise SystemExit(f"{name}: the fused mix is not the two mono mixes")
    for _ in range(5):
        fused()
        two_mono()
    pairs = {"fused": [], "two_mono": []}
    for _ in range(repeats):
        for which, fn in (("fused", fused), ("two_mono", two_mono)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            pairs[which].append((e0, e1))
    torch.cuda.synchronize()
    ms = {which: sorted(a.elapsed_time(b) for a, b in p) for which, p in pairs.items()}
    stats = {which: dict(median=v[len(v) // 2], min=v[0], max=v[-1]) for which, v in ms.items()}
    spans = np.array([min(h + r, total - o) for o, h, r, _, _ in table], dtype=np.int64)
    read, written = 4 * int(spans.sum()), 2 * 4 * total + 2 * 2 * total
    return dict(notes=len(kept), clip_seconds=total / RATE, mean_overlap=float(spans.sum()) / total,
                fused_ms=stats["fused"], two_mono_ms=stats["two_mono"], two_mono_over_fused=stats["two_mono"]["median"] / stats["fused"]["median"],
                fused_bytes=dict(read=read, written=written), fused_gb_per_s=(read + written) / stats["fused"]["median"] / 1e6,
                two_mono_bytes=dict(read=2 * read, written=written), joint_peak=float(peak[0]), side_peaks=[float(peak[1]), float(peak[2])])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ensemble.py measures on the GPU: no device found")
    torch.cuda.set_device(0)
    result = dict(config=dict(length=LENGTH, sample_rate=RATE, repeats=args.repeats, normalize=True, pcm=True),
                  sparse=measure("sparse", 200, 60.0, args.repeats), dense=measure("dense", 3000, 200.0, args.repeats))
    print(json.dumps(result))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
