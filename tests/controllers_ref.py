"""The rules of controllers (DESIGN.md "Controllers") restated in numpy float64 -- written from the rules, not from the kernel or from
gansynth_amd/notes.py: what gs_note_mix_curves, notes.read_performance, notes.schedule_curves and GANSynth.synthesize(controllers=True)
are held to.  The envelope, the table order and pcm16 are tests/synth_ref.py's, the finish is tests/stereo_ref.py's.

    pedal: a lane's pedal is down at time x when the last of its events at or before x (file order inside one time) is a down.  A note
    that ends under a pedal that is down ends at the first pedal-up after that, at the file's last event when none comes; never later than
    the next start, after its own, of a note of its (lane, pitch), nor than the file's last event; never earlier than written.
    curves: state (vol, expr, pan) from (100, 127, position); a = (vol / 127) (expr / 127); stereo target (a cos th, a sin th),
    th = (pan + 1) pi / 4; mono target (a, a), pan events ignored.  An event sits at sample floor(seconds sr + 0.5); the events of one
    sample count as the last of them.  Sample 0: the first value, no ramp.  A later sample s: a straight line from the curve's value
    at s to the new target at s + R, R = max(1, floor(ramp sr + 0.5)); a line still under way at s ends there.  Constant outside.
    curve_c(t): the straight line between the two points around t, the first / last value outside them.
    mix_c[t] = sum over the covering notes in table order of ((gain env(k)) curve_c(t)) waves[row][k]
"""
import math

import numpy as np

from tests import synth_ref as SRF


# ----------------------------------------------------------------------------------------------------------------- pedal
def pedal(notes, events, last):
    """notes: (lane, pitch, start, end) rows; events: lane -> [(time, down)] in deciding order; last: the file's last event.
    -> the new ends, one per note."""
    out = []
    for lane, pitch, start, end in notes:
        seq = events.get(lane, [])
        before = [down for time, down in seq if time <= end]
        if not before or not before[-1]:
            out.append(end)
            continue
        stop = last
        for time, down in seq:
            if time > end and not down:
                stop = time
                break
        for lane2, pitch2, start2, _ in notes:
            if (lane2, pitch2) == (lane, pitch) and start2 > start:
                stop = min(stop, start2)
        out.append(max(end, min(stop, last)))
    return out


# ---------------------------------------------------------------------------------------------------------------- curves
def target(vol, expr, pan, stereo):
    a = (vol / 127) * (expr / 127)
    if not stereo:
        return (a, a)
    th = (pan + 1) * math.pi / 4
    return (a * math.cos(th), a * math.sin(th))


def line(points, s):
    """The float64 polyline through (pos, l, r) rows at sample s, constant outside."""
    if s <= points[0][0]:
        return points[0][1:]
    for (p0, l0, r0), (p1, l1, r1) in zip(points, points[1:]):
        if p0 <= s < p1:
            x = (s - p0) / (p1 - p0)
            return (l0 + x * (l1 - l0), r0 + x * (r1 - r0))
    return points[-1][1:]


def curves(controls, positions, sample_rate, ramp_seconds, stereo):
    """controls: per part [(seconds, kind, value)] in time order; positions: the default pan per part.
    -> (points [(pos, fp32 l, fp32 r)], first)."""
    ramp = max(1, int(math.floor(ramp_seconds * sample_rate + 0.5)))
    points, first = [], [0]
    for events, position in zip(controls, positions):
        state = dict(volume=100, expression=127, pan=position)
        by_sample = {}
        for seconds, kind, value in events:
            if kind == "pan" and not stereo:
                continue
            state[kind] = value
            by_sample[int(math.floor(seconds * sample_rate + 0.5))] = dict(state)   # (the last one of a sample stays)
        begin = by_sample.pop(0, dict(volume=100, expression=127, pan=position))
        poly = [(0,) + target(begin["volume"], begin["expression"], begin["pan"], stereo)]
        for s in sorted(by_sample):
            here = line(poly, s)
            poly = [p for p in poly if p[0] < s] + [(s,) + tuple(here)]
            st = by_sample[s]
            poly.append((s + ramp,) + target(st["volume"], st["expression"], st["pan"], stereo))
        points += [(pos, np.float32(l), np.float32(r)) for pos, l, r in poly]
        first.append(len(points))
    return points, first


# ------------------------------------------------------------------------------------------------------------------- mix
def _part(points, first, p, c):
    rows = points[first[p]:first[p + 1]]
    return np.array([r[0] for r in rows], dtype=np.int64), np.array([r[1 + c] for r in rows], dtype=np.float32)


def curve(points, first, p, c, t):
    """curve_c of part p at the samples t (int64 array) -> (float64 values, V = the larger |value| of the two points around each t)."""
    pos, v = _part(points, first, p, c)
    v = v.astype(np.float64)
    i = np.searchsorted(pos, t, side="right") - 1
    lo, hi = np.clip(i, 0, len(pos) - 1), np.clip(i + 1, 0, len(pos) - 1)
    span = np.where(hi > lo, pos[hi] - pos[lo], 1).astype(np.float64)
    x = np.where((i >= 0) & (hi > lo), (t - pos[lo]) / span, 0.0)
    return v[lo] + x * (v[hi] - v[lo]), np.maximum(np.abs(v[lo]), np.abs(v[hi]))


def curve_f32(points, first, p, c, t):
    """The stated fp32 order: fl(v_i + fl(fl((float)(t - p_i) * fl(1 / (float)(p_i+1 - p_i))) * fl(v_i+1 - v_i)))."""
    pos, v = _part(points, first, p, c)
    i = np.searchsorted(pos, t, side="right") - 1
    inside = (i >= 0) & (i < len(pos) - 1)
    lo = np.clip(i, 0, len(pos) - 1)
    hi = np.where(inside, lo + 1, lo)
    d = np.where(inside, pos[hi] - pos[lo], 1).astype(np.float32)
    inv = (np.float32(1.0) / d).astype(np.float32)
    x = ((t - pos[lo]).astype(np.float32) * inv).astype(np.float32)
    dv = (v[hi] - v[lo]).astype(np.float32)
    return np.where(inside, (v[lo] + (x * dv).astype(np.float32)).astype(np.float32), v[lo]).astype(np.float32)


def _covered(row, total):
    onset, hold, release = row[:3]
    return min(hold + release, total - onset)


def mix(waves, table, points, first, total, channels):
    """table rows (onset, hold, release, row, gain, curve) -> (mix [channels, total], A [channels, total], M [total]) in float64 from the
    fp32 inputs.  A sums, per term, |gain env| * V * |sample| with V the larger of the two curve points around t -- what the interpolation's
    error is relative to (curve_c(t) itself may be near 0)."""
    waves = np.asarray(waves, dtype=np.float64)
    out, a, m = np.zeros((channels, total)), np.zeros((channels, total)), np.zeros(total, dtype=np.int64)
    for row in SRF._sorted(table):
        onset, hold, release, wave, gain, part = row
        n = _covered(row, total)
        if n <= 0:
            continue
        t = onset + np.arange(n, dtype=np.int64)
        ge = float(np.float32(gain)) * SRF.envelope(hold, release)[:n]
        for c in range(channels):
            value, big = curve(points, first, part, c, t)
            out[c, onset:onset + n] += (ge * value) * waves[wave, :n]
            a[c, onset:onset + n] += np.abs(ge) * big * np.abs(waves[wave, :n])
        m[onset:onset + n] += 1
    return out, a, m


def mix_f32(waves, table, points, first, total, channels):
    """The same sum in fp32, operation by operation in the order include/gansynth_hip.h states: tests/synth_ref.py's envelope and
    gain * env, then fl(. * curve_c(t)), fl(. * sample), the running sum."""
    waves = np.asarray(waves, dtype=np.float32)
    out = np.zeros((channels, total), dtype=np.float32)
    for row in SRF._sorted(table):
        onset, hold, release, wave, gain, part = row
        n = _covered(row, total)
        if n <= 0:
            continue
        k = np.arange(n)
        inv = np.float32(1.0) / np.float32(release + 1)
        env = np.where(k < hold, np.float32(1.0), (release - (k - hold)).astype(np.float32) * inv).astype(np.float32)
        ge = (np.float32(gain) * env).astype(np.float32)
        for c in range(channels):
            g = (ge * curve_f32(points, first, part, c, onset + k.astype(np.int64))).astype(np.float32)
            out[c, onset:onset + n] = out[c, onset:onset + n] + (g * waves[wave, :n]).astype(np.float32)
    return out


def bound(a, m):
    """|got - mix| <= (M + 12) * 2^-24 * A per sample and channel.  tests/synth_ref.py's bound, (M + 6) * 2^-24 * A, counts the
    envelope's one or two roundings, the two products and the M - 1 additions, with room.  The curve adds six roundings per term, each
    at most 2^-24 of the term's share of A when the curve's values are not negative (the gains of notes.schedule_curves never are), so
    that |v_i+1 - v_i| <= V = max(v_i, v_i+1):
        fl(v_i+1 - v_i): one, of a difference of at most V;
        x = fl(fl(t - p_i) * fl(1 / (p_i+1 - p_i))) in [0, 1]: the reciprocal and the product, two relative errors that reach the term
        through x * dv, again at most V each (both integer differences are below 2^24 here and convert exactly);
        fl(x * dv): one, of a product of at most V;
        fl(v_i + .): one, of a value between v_i and v_i+1, at most V;
        fl(fl(gain env) * curve): the one product the mix did not have.
    A is formed with V in place of curve_c(t), so every one of them is at most 2^-24 * A's term."""
    return (m + 12) * 2.0 ** -24 * a


# ------------------------------------------------------------------------------------------------- the dense case with curves
def dense_case():
    """tests/stereo_ref.py's dense table (40 notes, L = 1024, rows 1100 apart, total 9001: three tiles, the last partial) with one gain
    per note and part n % 5 -- neighbouring candidates change part -- and five curves:
      0  a point every few hundred samples, among them 4095, 4096 and 4097 (the tile edge) and 4200, 4201, 4202, 4203 (one lane's pack:
         4200 = 4096 + 4 * 26), which also gives segments of length 1
      1  one segment from 100 to 8900: it spans all three tiles
      2  one point
      3  first point at 3000 (after the first note), last at 6000 (before total)
      4  down to 0 at 4500, 0 until 5000, up again
    -> (waves [40, 1100] fp32, table rows (onset, hold, release, row, gain, curve), points, first)."""
    from tests import stereo_ref as STR
    waves, stereo = STR.dense_table()
    table = [row[:4] + (float(np.float32(math.hypot(row[4], row[5]))), n % 5) for n, row in enumerate(stereo)]
    f = np.float32
    curves_ = [
        [(0, 0.9, 0.1), (700, 0.2, 0.8), (4095, 0.75, 0.3), (4096, 0.7, 0.35), (4097, 0.1, 0.9), (4200, 0.6, 0.6), (4201, 0.61, 0.2),
         (4202, 0.3, 0.21), (4203, 0.31, 0.95), (6000, 1.0, 0.05), (8999, 0.4, 0.4)],
        [(100, 0.05, 1.0), (8900, 0.95, 0.15)],
        [(1234, 0.625, 0.375)],
        [(3000, 0.8, 0.3), (3500, 0.1, 0.9), (6000, 0.5, 0.55)],
        [(0, 0.7, 0.7), (4500, 0.0, 0.0), (5000, 0.0, 0.0), (5001, 0.5, 0.0), (7000, 0.2, 0.9)],
    ]
    points, first = [], [0]
    for rows in curves_:
        points += [(pos, float(f(l)), float(f(r))) for pos, l, r in rows]
        first.append(len(points))
    return waves, table, points, first
