"""Pitch bend restated in numpy (DESIGN.md "Pitch bend"): the reading of bend events into ratio curves, the coefficient table, the warp in
float64 (`warp_f64`) and its fp32 restatement in the stated order (`warp_f32`).  Library and Python are held to this file; nothing here
imports the package under test."""
import math

import numpy as np

Z, Q, BETA = 32, 256, 12.0
ZQ = Z * Q
HALF = 4 * Z            # taps on either side at the lowest cutoff (ratio 4)
PIECE = 160             # a ramp is cut into pieces of at most this many samples
RATIO_MIN, RATIO_MAX = 0.25, 4.0


# ---------------------------------------------------------------------------------------------------------------- curves
def _round(x):
    return int(math.floor(x + 0.5))


def curves(bends, sample_rate, ramp_seconds):
    """notes.schedule_bends restated: per part time-ordered (seconds, semitones) -> (points [(pos, ratio, cum)], first)."""
    ramp = max(1, _round(ramp_seconds * sample_rate))
    points, first = [], [0]
    for events in bends:
        groups = []
        for seconds, semitones in sorted(events, key=lambda e: e[0]):
            s = _round(seconds * sample_rate)
            if groups and groups[-1][0] == s:
                groups[-1][1] = float(semitones)
            else:
                groups.append([s, float(semitones)])
        if not groups:                                    # no bend event: no curve
            first.append(len(points))
            continue
        start = 0.0
        if groups[0][0] == 0:
            start = groups.pop(0)[1]
        curve = [(0, start)]
        for s, target in groups:
            v = curve[-1][1]
            if s < curve[-1][0]:                          # a ramp in progress: cut at its interpolated value
                (p0, v0), (p1, v1) = curve[-2], curve[-1]
                v = v0 + (s - p0) / (p1 - p0) * (v1 - v0)
                curve.pop()
            if s != curve[-1][0]:
                curve.append((s, v))
            curve.append((s + ramp, target))
        fine = [curve[0]]
        for (p0, v0), (p1, v1) in zip(curve, curve[1:]):
            if v0 != v1:
                for pos in range(p0 + PIECE, p1, PIECE):
                    fine.append((pos, v0 + (pos - p0) / (p1 - p0) * (v1 - v0)))
            fine.append((p1, v1))
        cum, rows = 0.0, []
        for i, (pos, semitones) in enumerate(fine):
            ratio = min(max(2.0 ** (semitones / 12.0), RATIO_MIN), RATIO_MAX)
            if i:
                p0, r0, _ = rows[-1]
                d = float(pos) - p0
                cum = cum + r0 * d + (ratio - r0) * d * d / (2.0 * d)
            rows.append((float(pos), ratio, cum))
        points += rows
        first.append(len(points))
    return points, first


def phi(points, t):
    """(Phi(t), ratio(t)) of one curve's points (rows (pos, ratio, cum)) at the samples t (an array), float64 in the stated order."""
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    t = np.asarray(t, dtype=np.float64)
    pos, ratio, cum = pts[:, 0], np.clip(pts[:, 1], RATIO_MIN, RATIO_MAX), pts[:, 2]
    k = np.searchsorted(pos, t, side="right")             # the first index whose pos is > t
    i0, i1 = np.maximum(k - 1, 0), np.minimum(k, len(pos) - 1)
    d, dp = t - pos[i0], pos[i1] - pos[i0]
    flat = (i0 == i1) | (k == 0) | ~(dp > 0)
    safe = np.where(flat, 1.0, dp)
    dr = ratio[i1] - ratio[i0]
    inside = cum[i0] + ratio[i0] * d + dr * d * d / (2.0 * safe)
    outside = cum[i0] + ratio[i0] * d
    return np.where(flat, outside, inside), np.where(flat, ratio[i0], ratio[i0] + dr * d / safe)


def positions(points, onset, count):
    """-> (n int64 [count], f fp32, c fp32) of a note: q = Phi(onset + k) - Phi(onset), n = floor(q), f = (float)(q - n), c = (float)min(1, 1 / r)."""
    t = float(onset) + np.arange(count, dtype=np.float64)
    p, r = phi(points, t)
    p0, _ = phi(points, np.array([float(onset)]))
    q = p - p0[0]
    n = np.floor(q)
    return n.astype(np.int64), (q - n).astype(np.float32), np.minimum(1.0, 1.0 / r).astype(np.float32)


# ----------------------------------------------------------------------------------------------------------------- table
def i0(x):
    q = 0.25 * x * x
    term = total = 1.0
    for k in range(1, 500):
        term *= q / (float(k) * float(k))
        total += term
        if term < 1e-17 * total:
            break
    return total


def table():
    """T[0 .. ZQ] and the zero that follows (ZQ + 2 entries), double rounded once to fp32, the exact 1 and 0s forced."""
    out = np.zeros(ZQ + 2, dtype=np.float32)
    i0b = i0(BETA)
    for m in range(ZQ + 1):
        if m % Q == 0:
            out[m] = 1.0 if m == 0 else 0.0
            continue
        x, a = m / Q, m / ZQ
        out[m] = np.float32(math.sin(math.pi * x) / (math.pi * x) * i0(BETA * math.sqrt(1.0 - a * a)) / i0b)
    return out


_TABLE = None


def _table():
    global _TABLE
    if _TABLE is None:
        _TABLE = table()
    return _TABLE


# ------------------------------------------------------------------------------------------------------------------ warp
def _taps(x, n):
    """x[n + j] for j in [-HALF + 1, HALF], zero outside the row: [count, 2 HALF]."""
    j = np.arange(-HALF + 1, HALF + 1)
    idx = n[:, None] + j[None]
    inside = (idx >= 0) & (idx < len(x))
    return np.where(inside, x[np.clip(idx, 0, len(x) - 1)], x.dtype.type(0)), j


def warp_f64(x, n, f, c, want_bound=False):
    """The rule from (n, f, c) on in float64: x fp32 [length]; f, c the fp32 values of `positions`; the table's fp32 entries.
    -> bent [count] float64, and with `want_bound` also B[k] = sum |h| |x[i]|."""
    T = _table().astype(np.float64)
    xs, j = _taps(np.asarray(x, dtype=np.float32).astype(np.float64), np.asarray(n))
    f64, c64 = np.asarray(f, dtype=np.float32).astype(np.float64), np.asarray(c, dtype=np.float32).astype(np.float64)
    a = np.minimum(c64[:, None] * np.abs(j[None].astype(np.float64) - f64[:, None]) * Q, float(ZQ))
    m = a.astype(np.int64)
    h = c64[:, None] * (T[m] + (a - m) * (T[m + 1] - T[m]))
    y = (h * xs).sum(axis=1)
    return (y, (np.abs(h) * np.abs(xs)).sum(axis=1)) if want_bound else y


def coefficients_f32(f, c):
    """h over the taps j in [-HALF + 1, HALF] in fp32, every operation rounded on its own: [count, 2 HALF]."""
    T = _table()
    f, c = np.asarray(f, dtype=np.float32), np.asarray(c, dtype=np.float32)
    j = np.arange(-HALF + 1, HALF + 1).astype(np.float32)
    a = np.minimum(c[:, None] * np.abs(j[None] - f[:, None]) * np.float32(Q), np.float32(ZQ))
    m = a.astype(np.int32)
    fr = a - m.astype(np.float32)
    return c[:, None] * (T[m] + fr * (T[m + 1] - T[m]))


def warp_f32(x, n, f, c):
    """fp32 in the stated order: the coefficients as above, products rounded, summed over ascending i one after the other."""
    xs, _ = _taps(np.asarray(x, dtype=np.float32), np.asarray(n))
    h = coefficients_f32(f, c)
    assert h.dtype == np.float32 and xs.dtype == np.float32
    acc = np.zeros(len(h), dtype=np.float32)
    for t in range(h.shape[1]):
        acc = acc + h[:, t] * xs[:, t]
    return acc


def warp_note(x, points, onset, count, precision="f64"):
    n, f, c = positions(points, onset, count)
    return (warp_f64 if precision == "f64" else warp_f32)(x, n, f, c)


def error_ratio(z, y64, bound):
    """e(z) = max |z - y64| / max B, pooled over all outputs of a case."""
    return float(np.abs(np.asarray(z, dtype=np.float64) - y64).max() / bound.max())


# ------------------------------------------------------------------------------------- the GPU test's inputs (tests/test_bend_gpu.py)
# tests/test_bend_cpu.py runs warp_f32 against warp_f64 on the same cases, so that the GPU tolerance exists before any device run.
LENGTH, STRIDE, ROWS, TILE = 3001, 3008, 6, 1024
SRC, SRC_B, DST, DST_B = 1, 1, 3, 5        # rows 0 and 2 are NaN, row 4 is a guard row of sentinels; both notes of a pair read row 1
SENTINEL = 12345.0
FAR = 3_000_000_007


def with_cum(rows):
    """(pos, ratio) rows of one curve -> (pos, ratio, cum) rows: cum by the stated formula, Phi measured from sample 0 under the first
    point's ratio."""
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


def source():
    """The source row: [LENGTH] fp32 in (-1, 1), no zero and so no negative zero."""
    rng = np.random.default_rng(23)
    x = (rng.random(LENGTH) * 2 - 1).astype(np.float32)
    x[x == 0] = np.float32(0.5)
    return x


def cases():
    """name -> (points, first, notes): notes are (src_row, dst_row, onset, count, curve)."""
    out = {}
    down = with_cum([(0, 2.0 ** (-1 / 12))])
    for count in (1, TILE - 1, TILE, TILE + 1, LENGTH):
        out[f"count {count}"] = (down, [0, 1], [(SRC, DST, 40, count, 0)])
    for name, ratio in (("0.25", 0.25), ("0.5", 0.5), ("1", 1.0), ("a semitone", 2.0 ** (1 / 12)), ("2", 2.0), ("4", 4.0)):
        out[f"ratio {name}"] = (with_cum([(0, ratio)]), [0, 1], [(SRC, DST, 7, LENGTH, 0)])
    inside = with_cum([(100, 1.0), (300, 1.3), (310, 0.8), (900, 0.8), (901, 1.9), (1500, 1.0)])
    out["segment ends inside one tile"] = (inside, [0, len(inside)], [(SRC, DST, 0, LENGTH, 0)])
    t = np.arange(0, 3200, 2)
    dense = with_cum(list(zip(t.tolist(), (2.0 ** (0.5 * np.sin(2 * np.pi * t / 400.0) / 12)).tolist())))
    out["a point every 2 samples"] = (dense, [0, len(dense)], [(SRC, DST, 11, LENGTH, 0)])
    through = with_cum([(0, 0.9), (2000, 1.1)])
    out["a ramp through 1"] = (through, [0, 2], [(SRC, DST, 0, LENGTH, 0)])
    far = with_cum([(FAR - 1000, 1.0), (FAR + 500, 1.25), (FAR + 1700, 0.7), (FAR + 5000, 1.0)])
    out["a far onset"] = (far, [0, len(far)], [(SRC, DST, FAR, LENGTH, 0)])
    shared = with_cum([(0, 1.0), (700, 1.2), (2500, 0.95)])
    out["two notes on one curve"] = (shared, [0, 3], [(SRC, DST, 0, LENGTH, 0), (SRC_B, DST_B, 500, 2000, 0)])
    before = with_cum([(10, 1.0), (50, 1.3)])
    out["no segment at the span"] = (before, [0, 2], [(SRC, DST, 5000, LENGTH, 0)])
    return out


def run_case(x, case, precision="f64"):
    """Every note of a case through the restatement -> [(y, y64, B)] per note, from the same fp32 f, c and table."""
    points, first, notes = case
    out = []
    for _, _, onset, count, curve in notes:
        n, f, c = positions(points[first[curve]:first[curve + 1]], onset, count)
        y64, bound = warp_f64(x, n, f, c, want_bound=True)
        out.append((y64 if precision == "f64" else warp_f32(x, n, f, c), y64, bound))
    return out
