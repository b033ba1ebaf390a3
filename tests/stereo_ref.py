"""The rules of parts and stereo (DESIGN.md "Parts and stereo") restated in numpy float64 -- written from the rules, not from the kernel or
from gansynth_amd/notes.py: what gs_note_mix_stereo, gs_stereo_finish, notes.schedule_gains and GANSynth.synthesize(stereo=True) are held to.
The mono rules (envelope, mix, bound, pcm16) are tests/synth_ref.py's, used as they are.

    g = (velocity / 127) (volume / 127),  theta = (pan + 1) pi / 4,  gain_l = fl32(g cos theta),  gain_r = fl32(g sin theta)
    a note without a pan: pan = spread (2 p / (Q - 1) - 1), p its part's rank among the Q parts with no pan anywhere (0 when Q == 1;
    0 as well for a part that is panned elsewhere)
    mix_c[t] = sum over the covering notes in table order of (gain_c env(k)) waves[row][k]
    peak = max over c, t of |mix_c[t]|;  out = fl32(mix / peak) when normalising and peak > 1;  pcm[t][c] = pcm16(out[c][t])
"""
import math

import numpy as np

from tests import synth_ref as SRF


def gains(velocity, volume, pan, part, n_parts, spread):
    """Per-note lists -> [(gain_l, gain_r)] as fp32 values.  `pan`: floats or None."""
    panned = {p for p, x in zip(part, pan) if x is not None}
    free = [p for p in range(n_parts) if p not in panned]
    out = []
    for vel, vol, x, p in zip(velocity, volume, pan, part):
        if x is None:
            x = spread * (2 * free.index(p) / (len(free) - 1) - 1) if p in free and len(free) > 1 else 0.0
        g = (vel / 127) * (vol / 127)
        theta = (x + 1) * math.pi / 4
        out.append((np.float32(g * math.cos(theta)), np.float32(g * math.sin(theta))))
    return out


def side(table, c):
    """Rows (onset, hold, release, row, gain_l, gain_r) -> the mono table of channel c."""
    return [tuple(row[:4]) + (row[4 + c],) for row in table]


def mix(waves, table, total):
    """-> (mix [2, total], A [2, total], M [total]) in float64: tests/synth_ref.py's mix of each side."""
    left, a_l, m = SRF.mix(waves, side(table, 0), total)
    right, a_r, _ = SRF.mix(waves, side(table, 1), total)
    return np.stack([left, right]), np.stack([a_l, a_r]), m


def mix_f32(waves, table, total):
    return np.stack([SRF.mix_f32(waves, side(table, c), total) for c in (0, 1)])


def finish(x, normalize):
    """x [2, n] fp32 -> (peak fp32, out [2, n] fp32, pcm [n, 2] int16): one peak over both rows, the quotient correctly rounded (the
    float64 quotient of two fp32 values, rounded once more to fp32, is the correctly rounded fp32 quotient: 53 >= 2 * 24 + 2)."""
    x = np.asarray(x, dtype=np.float32)
    peak = np.float32(np.abs(x).max())
    out = x
    if normalize and peak > 1:
        out = (x.astype(np.float64) / np.float64(peak)).astype(np.float32)
    return peak, out, np.ascontiguousarray(SRF.pcm16(out).T)


# --------------------------------------------------------------------------------------------------- the dense stereo case
TOTAL = 9001                  # three tiles of 4096, the last one partial; 9001 % 4 == 1
LENGTH, STRIDE = 1024, 1100   # waves rows of 1024 samples, 1100 apart


def dense_table(seed=21, count=40, total=TOTAL, lean=0.5):
    """40 notes of length <= 1024 in a clip of `total` samples, two thirds of them crowded into 1500 samples around the first tile edge (a
    dozen on one sample), the rest anywhere; gains up to 1 on either side, `lean` > 0.5 favouring the right.  -> (waves [40, 1100] fp32 of
    which [:, :1024] count, table rows (onset, hold, release, row, gain_l, gain_r))."""
    rng = np.random.default_rng(seed)
    waves = (rng.random((count, STRIDE)) * 2 - 1).astype(np.float32)
    table = []
    for n in range(count):
        onset = int(rng.integers(3300, 4800)) if n % 3 else int(rng.integers(0, total - 1))
        hold = int(np.exp(rng.uniform(np.log(8.0), np.log(LENGTH))))
        release = int(min(rng.integers(0, 400), LENGTH - hold))
        g, pan = float(rng.uniform(0.3, 1.0)), float(np.clip(rng.uniform(-1.2, 1.2) + (lean - 0.5) * 2, -1, 1))
        theta = (pan + 1) * math.pi / 4
        table.append((onset, hold, release, n, float(np.float32(g * math.cos(theta))), float(np.float32(g * math.sin(theta)))))
    table.sort(key=lambda r: r[0])
    return waves, table
