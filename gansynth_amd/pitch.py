"""Pitch of a note from its waveform: a YIN fundamental-frequency tracker (de Cheveigne & Kawahara 2002, steps 1-5) on HIP kernels
(csrc/yin.hip) and the note statistics built on it.  No classifier is involved: the figures say whether the AUDIO sounds at the pitch it was
asked for, in cents, and how steadily.

The rules below are this project's own statement of the method (include/gansynth_hip.h, DESIGN.md "Pitch tracking on the device"), and
tests/yin_ref.py restates every one in float64 numpy.  Rate 16 kHz; production parameters window W = 1024, lags L = 512, hop 256,
tau_min 8, threshold 0.15 (pitches 24 .. 84 have periods of 489.3 down to 15.3 samples).  A row of n samples has
F = (n - W - L) // hop + 1 frames (245 for n = 64000); frame f starts at t = f hop.

  1. Difference    d(tau) = sum_{j < W} (x[t + j] - x[t + j + tau])^2, the direct form, fp32; d(0) = 0.  Frame power p = (1 / W) sum x[t + j]^2.
  2. Normalisation in float64: S(tau) = d(1) + ... + d(tau) added in ascending order; c(0) = 1, c(tau) = d(tau) tau / S(tau), 1 where S = 0.
  3. Pick          over [tau_min, L - 2]: the first tau with c < threshold, then down to the local minimum (while c(tau + 1) < c(tau));
                   nothing under the threshold: the argmin, the lowest index on a tie.
  4. Parabola      den = c- - 2 c0 + c+; offset = 0.5 (c- - c+) / den clamped to [-1, 1] if den > 0, else 0; period = tau + offset;
                   aperiodicity = c(tau).
  5. Note          (host, float64) a frame is voiced iff its aperiodicity < threshold and its power > 1e-4 x the note's largest frame power;
                   cents = 1200 log2((rate / period) / f_label), f_label = 440 2^((p - 69) / 12); the note's deviation is the median of its
                   voiced frames' cents, its jitter their standard deviation; a note without a voiced frame is unvoiced (NaN).

YIN is not perfect on real instruments (bass notes whose period nears the lag range, mallets whose partials are inharmonic): the figures of a
generated set are to be read against the same figures of the real set, which GANSynth.evaluate(f0=True) returns beside them."""
import collections

import numpy as np
import torch

from . import kernels

WINDOW, LAGS, HOP, TAU_MIN, THRESHOLD = 1024, 512, 256, 8, 0.15
POWER_GATE = 1.0e-4          # a voiced frame's power, relative to the note's largest
ACCURATE_CENTS = 50.0        # a note is accurate when |median cents| is below this: the nearest semitone is the label

Track = collections.namedtuple("Track", "lag period aperiodicity power")
NoteStatistics = collections.namedtuple("NoteStatistics", "cents jitter voiced")


def track(waveforms, window=WINDOW, lags=LAGS, hop=HOP, tau_min=TAU_MIN, threshold=THRESHOLD):
    """waveforms [rows, n] (fp32 on the device; [n]: one row) -> Track(lag int32, period float64, aperiodicity float64, power fp32), device
    tensors [rows, frames], from ONE gs_yin_track call."""
    if not isinstance(waveforms, torch.Tensor):
        raise ValueError(f"track: waveforms must be a tensor (got {type(waveforms).__name__})")
    x = waveforms[None] if waveforms.dim() == 1 else waveforms
    if x.dtype != torch.float32 and x.is_floating_point():
        x = x.float()
    return Track(*kernels.yin_track(x, window, lags, hop, tau_min, threshold))


def label_frequency(pitches):
    """MIDI pitch -> Hz, float64: 440 2^((p - 69) / 12)."""
    return 440.0 * 2.0 ** ((np.asarray(pitches, dtype=np.float64) - 69.0) / 12.0)


def _host(t, dtype=np.float64):
    return (t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)).astype(dtype)


def note_statistics(period, aperiodicity, power, pitches, rate=16000, threshold=THRESHOLD):
    """Rule 5 in numpy float64.  period, aperiodicity, power: [notes, frames] (tensors or arrays); pitches: [notes] MIDI numbers.
    -> NoteStatistics(cents [notes] float64: the median deviation of the voiced frames, NaN for an unvoiced note; jitter [notes]: their
    standard deviation, NaN likewise; voiced [notes] int64: the voiced frames)."""
    period, aper, power = _host(period), _host(aperiodicity), _host(power)
    pitches = np.asarray(pitches, dtype=np.float64).reshape(-1)
    if period.ndim != 2 or period.shape != aper.shape or period.shape != power.shape or period.shape[0] != pitches.shape[0]:
        raise ValueError(f"note_statistics: period, aperiodicity and power must be [notes, frames] alike and pitches [notes] "
                         f"(got {period.shape}, {aper.shape}, {power.shape}, {pitches.shape})")
    notes = period.shape[0]
    cents, jitter, voiced = np.full(notes, np.nan), np.full(notes, np.nan), np.zeros(notes, dtype=np.int64)
    f_label = label_frequency(pitches)
    for i in range(notes):
        mask = (aper[i] < threshold) & (power[i] > POWER_GATE * power[i].max())
        voiced[i] = int(mask.sum())
        if voiced[i]:
            c = 1200.0 * np.log2((float(rate) / period[i][mask]) / f_label[i])
            cents[i], jitter[i] = np.median(c), np.std(c)
    return NoteStatistics(cents, jitter, voiced)


def fold_cents(cents):
    """Cents folded to [-600, 600): an octave error becomes 0."""
    return (np.asarray(cents, dtype=np.float64) + 600.0) % 1200.0 - 600.0


def summarize(cents, jitter):
    """Per-note cents and jitter (NaN: unvoiced) -> the five figures: f0_pitch_accuracy (the share of ALL notes with |cents| < 50),
    f0_chroma_accuracy (the same with the cents folded to +-600: octave errors are the gap between the two), f0_median_abs_cents (the median
    |cents| over the notes counted accurate), f0_jitter_cents (the mean jitter over the same notes) and f0_voiced_fraction.  The two figures
    over the accurate notes are NaN when there is none."""
    cents, jitter = np.asarray(cents, dtype=np.float64).reshape(-1), np.asarray(jitter, dtype=np.float64).reshape(-1)
    if cents.shape != jitter.shape or cents.size == 0:
        raise ValueError(f"summarize: cents and jitter must be non-empty vectors alike (got {cents.shape}, {jitter.shape})")
    voiced = ~np.isnan(cents)
    with np.errstate(invalid="ignore"):
        accurate = voiced & (np.abs(cents) < ACCURATE_CENTS)
        chroma = voiced & (np.abs(fold_cents(cents)) < ACCURATE_CENTS)
    return dict(f0_pitch_accuracy=float(accurate.mean()), f0_chroma_accuracy=float(chroma.mean()),
                f0_median_abs_cents=float(np.median(np.abs(cents[accurate]))) if accurate.any() else float("nan"),
                f0_jitter_cents=float(jitter[accurate].mean()) if accurate.any() else float("nan"),
                f0_voiced_fraction=float(voiced.mean()))


class NoteAccumulator(object):
    """Per-note results batch by batch (GANSynth.evaluate): add(waveforms, pitches) tracks one batch and keeps its notes' cents and jitter --
    a few numbers a note; the waveforms are not kept."""

    def __init__(self, rate=16000, **track_args):
        self.rate, self.track_args = rate, track_args
        self.cents, self.jitter = [], []

    def add(self, waveforms, pitches):
        t = track(waveforms, **self.track_args)
        stats = note_statistics(t.period, t.aperiodicity, t.power, pitches, rate=self.rate, threshold=self.track_args.get("threshold", THRESHOLD))
        self.cents.append(stats.cents)
        self.jitter.append(stats.jitter)

    def result(self):
        """-> (the five figures, cents [notes], jitter [notes])."""
        if not self.cents:
            raise ValueError("NoteAccumulator: no batch was added")
        cents, jitter = np.concatenate(self.cents), np.concatenate(self.jitter)
        return summarize(cents, jitter), cents, jitter
