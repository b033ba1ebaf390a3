"""The sustain rules (DESIGN.md "Sustain") restated in numpy -- written from the rules, not from the kernels or from gansynth_amd/notes.py:
this module is what gs_loop_search, gs_note_sustain, notes.sustain_plan, notes.pick_loop, notes.schedule_sustain and
GANSynth.synthesize(sustain=True) are held to.

    The plan, for notes of L samples:  a = 3 L // 8,  m in [L // 8, L // 4],  W = max(16, L // 32),  X = max(1, L // 64);  L >= 64.
    The score of a lag m, x the note's row:  S_aa = sum_{i<W} x[a+i]^2,  S_ab = sum_{i<W} x[a+i] x[a+m+i],  S_bb = sum_{i<W} x[a+m+i]^2,
        score(m) = S_ab / sqrt(S_aa S_bb), or 0 where S_aa S_bb == 0.
    The pick: non-finite scores count as -inf; m* = the LARGEST lag with score >= max - tie; all scores -inf or 0: m* = the last lag.
    The waveform, b = a + m:  y[k] = x[k] (k < b);  beyond, p = (k - b) mod m:  y[k] = (1 - w) x[b + p] + w x[a + p] with
        w = (p + 1) / (X + 1) where p < X, and y[k] = x[a + p] otherwise.
    The schedule:  hold = max(1, floor((end - start) sr + 0.5)), unclamped;  held iff hold + R > L;  pieces of L while more than L remains,
        a remainder r <= L - R the last piece, a longer one split into r - (L - R) and L - R;  only the last piece has the release R.
"""
import math

import numpy as np

from tests import synth_ref as SR


def sustain_plan(length):
    if length < 64:
        raise ValueError("L < 64")
    return 3 * length // 8, length // 8, length // 4, max(16, length // 32), max(1, length // 64)


# ------------------------------------------------------------------------------------------------------------- the search
def scores_f64(x, a, m_min, m_max, window):
    """score(m) for m in [m_min, m_max] in float64 from the fp32 row."""
    x = np.asarray(x, dtype=np.float64)
    u = x[a:a + window]
    s_aa = float(np.dot(u, u))
    out = np.zeros(m_max - m_min + 1)
    for j, m in enumerate(range(m_min, m_max + 1)):
        v = x[a + m:a + m + window]
        s_ab, s_bb = float(np.dot(u, v)), float(np.dot(v, v))
        out[j] = s_ab / math.sqrt(s_aa * s_bb) if s_aa * s_bb != 0 else 0.0
    return out


def scores_f32(x, a, m_min, m_max, window):
    """The same in fp32 in a plain order: the three sums tap by tap from i = 0, every product and every addition rounded on its own,
    then the product of the two energies, its square root and the quotient."""
    x = np.asarray(x, dtype=np.float32)
    lags = np.arange(m_min, m_max + 1)
    s_aa = np.float32(0)
    s_ab, s_bb = np.zeros(len(lags), dtype=np.float32), np.zeros(len(lags), dtype=np.float32)
    for i in range(window):
        u, v = x[a + i], x[a + lags + i]
        s_aa = np.float32(s_aa + np.float32(u * u))
        s_ab = (s_ab + (u * v).astype(np.float32)).astype(np.float32)
        s_bb = (s_bb + (v * v).astype(np.float32)).astype(np.float32)
    prod = (s_aa * s_bb).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(prod == 0, np.float32(0), s_ab / np.sqrt(prod)).astype(np.float32)


def pick_loop(scores, m_min, tie=1e-3):
    s = np.array(scores, dtype=np.float64)
    s[~np.isfinite(s)] = -np.inf
    if all(v == 0 or v == -np.inf for v in s):
        return m_min + len(s) - 1
    return m_min + max(j for j, v in enumerate(s) if v >= s.max() - tie)


# ----------------------------------------------------------------------------------------------------------- the waveform
def _indices(offset, count, a, m):
    k = offset + np.arange(count, dtype=np.int64)
    b = a + m
    p = np.where(k >= b, (k - b) % m, 0)
    return k, b, p


def sustained_f64(x, a, m, xfade, offset, count):
    """y[offset : offset + count] in float64 from the fp32 row."""
    x = np.asarray(x, dtype=np.float64)
    k, b, p = _indices(offset, count, a, m)
    w = (p + 1) / (xfade + 1.0)
    fade = p < xfade
    looped = np.where(fade, (1.0 - w) * x[np.where(fade, b + p, 0)] + w * x[a + p], x[a + p])
    return np.where(k < b, x[np.minimum(k, b - 1)], looped)


def sustained_f32(x, a, m, xfade, offset, count):
    """The same in fp32, every operation rounded on its own and in the order written: fl(1 / (X + 1)), w = (float)(p + 1) * that, 1 - w,
    the two products, their sum.  gs_note_sustain computes exactly this."""
    x = np.asarray(x, dtype=np.float32)
    k, b, p = _indices(offset, count, a, m)
    inv = np.float32(1.0) / np.float32(xfade + 1)
    w = ((p + 1).astype(np.float32) * inv).astype(np.float32)
    fade = p < xfade
    one = ((np.float32(1.0) - w).astype(np.float32) * x[np.where(fade, b + p, 0)]).astype(np.float32)
    two = (w * x[a + p]).astype(np.float32)
    looped = np.where(fade, (one + two).astype(np.float32), x[a + p])
    return np.where(k < b, x[np.minimum(k, b - 1)], looped).astype(np.float32)


# ----------------------------------------------------------------------------------------------------------- the schedule
def pieces(hold, full, length):
    """[(offset, hold_s, release_s)] of a held note: hold + full > length, full <= length - 1."""
    out, offset = [], 0
    while hold - offset > length:
        out.append((offset, length, 0))
        offset += length
    r = hold - offset
    if r <= length - full:
        return out + [(offset, r, full)]
    first = r - (length - full)
    return out + [(offset, first, 0), (offset + first, length - full, full)]


def schedule_sustain(notes, pitches, sample_rate, length, release_seconds, cut=()):
    """notes: (pitch, velocity, start, end) rows -> (table, T, indices of the kept notes, dropped, owner, offset): synth_ref.schedule's
    rows for the notes that are not held (or are in `cut`, by kept index), one row per piece for the held ones, their rows counted on
    from the number of kept notes; owner: the kept note of each table entry; offset: the piece's offset, None for an ordinary row."""
    base, total, kept, dropped = SR.schedule(notes, pitches, sample_rate, length, release_seconds)
    full = int(math.floor(release_seconds * sample_rate + 0.5))
    if full > length - 1:
        raise ValueError("R > L - 1")
    table, owner, offset, row = [], [], [], len(kept)
    for n, i in enumerate(kept):
        _, velocity, start, end = notes[i]
        hold = max(1, int(math.floor((end - start) * sample_rate + 0.5)))
        if hold + full <= length or n in cut:
            table.append(base[n])
            owner.append(n)
            offset.append(None)
            continue
        for off, h, r in pieces(hold, full, length):
            table.append((base[n][0] + off, h, r, row, velocity / 127))
            owner.append(n)
            offset.append(off)
            row += 1
    return table, max(o + h + r for o, h, r, _, _ in table), kept, dropped, owner, offset


def piece_rows(waves, table, owner, offset, loops, a, xfade, kind="f64"):
    """The waves buffer the mix reads: the given rows, then one row per piece, cut from the looped waveform of its note (loops: kept
    note -> m) and zero beyond the piece's samples."""
    length = waves.shape[1]
    make, dtype = (sustained_f64, np.float64) if kind == "f64" else (sustained_f32, np.float32)
    extra = []
    for (onset, hold, release, row, _), n, off in zip(table, owner, offset):
        if off is None:
            continue
        assert row == len(waves) + len(extra)
        y = np.zeros(length, dtype=dtype)
        y[:hold + release] = make(waves[n], a, loops[n], xfade, off, hold + release)
        extra.append(y)
    return np.concatenate([np.asarray(waves, dtype=dtype), np.asarray(extra, dtype=dtype).reshape(-1, length)])


def mix_long_f64(x, a, m, xfade, onset, hold, release, gain, total):
    """One note that runs hold + release samples of its looped waveform under the note-mix envelope, in float64 -> [total]."""
    out = np.zeros(total)
    n = min(hold + release, total - onset)
    y = sustained_f64(x, a, m, xfade, 0, hold + release)
    out[onset:onset + n] = ((float(np.float32(gain)) * SR.envelope(hold, release)) * y)[:n]
    return out


# -------------------------------------------------------------------------------------------------------- the test tones
LENGTH, STRIDE = 3001, 3008
TONE_PLAN = (900, 400, 900, 256)            # a, m_min, m_max, W of the tests on the tones (plan-like, fixed)
TONE_XFADE = 64
PERIODS = (37.3, 50.0, 61.7, 122.4)
SENTINEL = -77.25


def tone(period, length=LENGTH, seed=5):
    """Five harmonics with amplitude 1 / h, decaying as exp(-n / 6000), plus 1e-3 of seeded noise, as fp32."""
    n = np.arange(length, dtype=np.float64)
    x = sum(np.sin(2 * np.pi * h * n / period) / h for h in range(1, 6)) * np.exp(-n / 6000.0)
    return (x + 1e-3 * np.random.default_rng(seed).standard_normal(length)).astype(np.float32)


def search_rows(length=LENGTH):
    """The four tones, a silent row and a noise row: [6, length] fp32."""
    rows = [tone(p, length) for p in PERIODS]
    rows.append(np.zeros(length, dtype=np.float32))
    rows.append(np.random.default_rng(9).standard_normal(length).astype(np.float32))
    return np.stack(rows)
