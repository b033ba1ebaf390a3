"""True peak of rendered clips: the peak of the reconstructed waveform in dBTP, measured on a 4x oversampled signal as ITU-R BS.1770-4 Annex 2
describes it (not in the reference; the rule is this project's own, DESIGN.md "True peak").

A clip whose samples all stay under a ceiling can still reconstruct above it in a DAC or a lossy encoder: between two samples the waveform
goes where the samples do not.  Loudness delivery specifications (EBU R128: -1 dBTP) therefore state the ceiling as a true peak.  The detector
is the project's own 1 -> 4 resampler design (68 taps a phase), evaluated on the device without ever writing the 4x signal
(kernels.true_peak, gs_true_peak); `limiter.apply(..., true_peak=True)` and `loudness.apply(..., true_peak=True)` feed its envelope to the limiter.

    measure(clip) -> dBTP of a [n] or [2, n] fp32 device clip; -inf for silence
"""
import math

import torch

from . import _lib

OVERSAMPLE = _lib.TRUE_PEAK_OVERSAMPLE


def to_db(peak):
    """20 log10 of a linear peak; -inf for 0."""
    peak = float(peak)
    return 20.0 * math.log10(peak) if peak > 0 else -math.inf


def measure(clip):
    """The true peak in dBTP (relative to full scale 1.0) of clip ([n] or [2, n] fp32 on the device): one detector call, no envelope."""
    from . import kernels
    if not isinstance(clip, torch.Tensor) or clip.dim() not in (1, 2) or clip.dtype != torch.float32 or clip.numel() == 0 or \
            (clip.dim() == 2 and clip.shape[0] != 2):
        got = f"{tuple(clip.shape)} {clip.dtype}" if isinstance(clip, torch.Tensor) else type(clip).__name__
        raise ValueError(f"true_peak.measure: clip must be [n] or [2, n] fp32 (got {got})")
    return to_db(kernels.true_peak(clip, want_envelope=False)[1])
