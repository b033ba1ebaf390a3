"""The note-sequence rules (DESIGN.md "Note sequences") restated in numpy float64 -- written from the rules, not from the kernel or from
gansynth_amd/notes.py: this module is what gs_note_mix, kernels.note_mix, notes.schedule and GANSynth.synthesize are held to.

    sr = sample_rate, L = waveform_length, R = floor(release_seconds * sr + 0.5); per note, in (start, appearance) order:
    onset = floor(start * sr + 0.5)   hold = clamp(floor((end - start) * sr + 0.5), 1, L)   release = min(R, L - hold)   gain = velocity / 127
    T = max(onset + hold + release)
    env(k) = 1 (k < hold),  (release - (k - hold)) / (release + 1) (hold <= k < hold + release),  0 beyond
    mix[t] = sum over the notes with onset <= t < onset + hold + release, in table order, of (gain * env(t - onset)) * waves[row][t - onset]
"""
import math

import numpy as np


def schedule(notes, pitches, sample_rate, waveform_length, release_seconds):
    """notes: (pitch, velocity, start, end) rows -> (table rows (onset, hold, release, row, gain), T, indices of the kept notes, dropped)."""
    table_pitches = sorted(pitches)
    full = int(math.floor(release_seconds * sample_rate + 0.5))
    order = sorted(range(len(notes)), key=lambda i: (notes[i][2], i))
    table, kept = [], []
    for i in order:
        pitch, velocity, start, end = notes[i]
        if pitch not in table_pitches:
            continue
        onset = int(math.floor(start * sample_rate + 0.5))
        hold = int(math.floor((end - start) * sample_rate + 0.5))
        hold = max(1, min(hold, waveform_length))
        release = min(full, waveform_length - hold)
        table.append((onset, hold, release, len(kept), velocity / 127))
        kept.append(i)
    if not kept:
        raise ValueError("no note is left")
    total = max(o + h + r for o, h, r, _, _ in table)
    return table, total, kept, len(notes) - len(kept)


def envelope(hold, release):
    """env over k = 0 .. hold + release - 1 (float64)."""
    k = np.arange(hold + release, dtype=np.float64)
    return np.where(k < hold, 1.0, (release - (k - hold)) / (release + 1.0))


def _sorted(table):
    return [table[i] for i in sorted(range(len(table)), key=lambda i: (table[i][0], i))]


def mix(waves, table, total):
    """-> (mix [total], A = sum |term| per sample, M = covering notes per sample), float64 from the fp32 inputs (gain as the fp32 the
    kernel is handed).  Notes are clipped at `total`."""
    waves = np.asarray(waves, dtype=np.float64)
    out, a, m = np.zeros(total), np.zeros(total), np.zeros(total, dtype=np.int64)
    for onset, hold, release, row, gain in _sorted(table):
        n = min(hold + release, total - onset)
        if n <= 0:
            continue
        term = (float(np.float32(gain)) * envelope(hold, release)[:n]) * waves[row, :n]
        out[onset:onset + n] += term
        a[onset:onset + n] += np.abs(term)
        m[onset:onset + n] += 1
    return out, a, m


def mix_f32(waves, table, total):
    """The same sum carried out in fp32 in the stated order, every operation rounded on its own: fl(1 / (release + 1)), the envelope's
    product, gain * env, the product with the sample, the running sum.  (The kernel computes exactly this: tests/test_notes_gpu.py and
    tests/test_ensemble_gpu.py hold both channel counts to it bit for bit; on the CPU it shows how far an honest fp32 evaluation sits
    inside the bound of the float64 comparison.)"""
    waves = np.asarray(waves, dtype=np.float32)
    out = np.zeros(total, dtype=np.float32)
    for onset, hold, release, row, gain in _sorted(table):
        n = min(hold + release, total - onset)
        if n <= 0:
            continue
        k = np.arange(n)
        inv = np.float32(1.0) / np.float32(release + 1)
        env = np.where(k < hold, np.float32(1.0), (release - (k - hold)).astype(np.float32) * inv).astype(np.float32)
        ge = (np.float32(gain) * env).astype(np.float32)
        out[onset:onset + n] = out[onset:onset + n] + (ge * waves[row, :n]).astype(np.float32)
    return out


def bound(a, m):
    """|got - mix| <= (M + 6) * 2^-24 * A per sample: one or two roundings for the envelope, two for the products and M - 1 for the
    additions, each at most 2^-24 of A, with room for a reciprocal multiply and for contraction to fma."""
    return (m + 6) * 2.0 ** -24 * a


def slerp(a, b, t):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    omega = math.acos(min(1.0, max(-1.0, float(np.dot(a / np.sqrt(np.dot(a, a)), b / np.sqrt(np.dot(b, b)))))))
    if math.sin(omega) < 1e-6:
        return (1 - t) * a + t * b
    return math.sin((1 - t) * omega) / math.sin(omega) * a + math.sin(t * omega) / math.sin(omega) * b


def note_latents(anchors, starts, seconds_per_instrument):
    """anchors [K + 1, Z] at times j * seconds_per_instrument -> one fp32 latent per start (seconds)."""
    out = []
    for start in starts:
        j = int(math.floor(start / seconds_per_instrument))
        out.append(slerp(anchors[j], anchors[j + 1], start / seconds_per_instrument - j))
    return np.asarray(out).astype(np.float32)


def pcm16(x):
    """gs_summary_audio_s16's rule: clamp(round-half-away(x * 32768), -32768, 32767), NaN -> 0."""
    x = np.asarray(x, dtype=np.float32)
    y = x.astype(np.float64) * 32768.0
    r = np.clip(np.sign(y) * np.floor(np.abs(y) + 0.5), -32768, 32767)
    return np.where(np.isnan(x), 0, r).astype(np.int16)


# ------------------------------------------------------------------------------------------------- the dense random case
SR, L, RELEASE = 16000, 1024, 160


def dense_case(seed=7, count=40):
    """40 notes with onsets in [0, 0.2 s), holds from 8 samples to beyond L (log-uniform to 4 L), R = 160 samples, every pitch in the
    table: -> (waves [count, L] fp32, notes).  Deep overlaps, clamped holds and cut releases (the tests assert that the draw has them)."""
    rng = np.random.default_rng(seed)
    waves = (rng.random((count, L)) * 2 - 1).astype(np.float32)
    notes = []
    for _ in range(count):
        start = float(rng.random() * 0.2)
        samples = float(np.exp(rng.uniform(np.log(8.0), np.log(4.0 * L))))
        notes.append((int(rng.integers(24, 85)), int(rng.integers(1, 128)), start, start + samples / SR))
    return waves, notes
