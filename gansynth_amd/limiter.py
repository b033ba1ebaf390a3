"""Look-ahead limiter for rendered clips (not in the reference; the rule is this project's own, DESIGN.md "Limiter").

The last stage of a rendered score: mix -> resample -> reverb -> limiter -> PCM.  Instead of dividing the whole clip by its loudest sample,
the clip is scaled so that its peak would stand `drive_db` above the ceiling, and a smooth gain -- the sliding mean of a sliding minimum
over the look-ahead -- pulls back only the peaks.  No sample leaves the stage above the ceiling, so the 16-bit file cannot clip.

Host code, except `apply`'s call into kernels.limit (gs_limit on the device).

    design(rate, ceiling_db, drive_db, lookahead_seconds, peak)   -> (pre_gain, ceiling, lookahead in samples): host arithmetic
    apply(clip, rate, ...)                                         -> (out, pcm or None, peak, min_gain) of kernels.limit

`apply(..., true_peak=True)` reads the ceiling in dBTP: the clip's 4x oversampled envelope (kernels.true_peak, DESIGN.md "True peak") sets the
pre-gain and goes to the kernel, which then holds the reconstructed waveform, not only the samples, under the ceiling.
"""
import math

import numpy as np
import torch

from . import _lib

MAX_LOOKAHEAD = _lib.LIMIT_MAX_LOOKAHEAD


def _number(name, v):
    if not isinstance(v, (int, float, np.integer, np.floating)) or isinstance(v, bool) or not math.isfinite(v):
        raise ValueError(f"limiter: {name} must be a finite number (got {v!r})")
    return float(v)


def lookahead_samples(rate, lookahead_seconds):
    """W = floor(lookahead_seconds * rate + 0.5), at least 1; beyond MAX_LOOKAHEAD samples the request is refused."""
    if not (isinstance(rate, (int, np.integer)) and not isinstance(rate, bool)) or rate <= 0:
        raise ValueError(f"limiter: rate must be a positive integer (got {rate!r})")
    seconds = _number("lookahead_seconds", lookahead_seconds)
    if seconds < 0:
        raise ValueError(f"limiter: lookahead_seconds must not be negative (got {lookahead_seconds!r})")
    w = int(math.floor(seconds * int(rate) + 0.5))
    if w > MAX_LOOKAHEAD:
        raise ValueError(f"limiter: lookahead_seconds {seconds} at {rate} Hz is {w} samples, more than {MAX_LOOKAHEAD}: the longest "
                         f"look-ahead at this rate is {MAX_LOOKAHEAD / int(rate):.6f} seconds")
    return max(w, 1)


def design(rate, ceiling_db=-1.0, drive_db=6.0, lookahead_seconds=0.005, peak=1.0):
    """-> (pre_gain, ceiling, W).  ceiling c = 10 ** (ceiling_db / 20), ceiling_db <= 0; pre_gain = c * 10 ** (drive_db / 20) / peak,
    drive_db >= 0 -- `peak` is the clip's own: scaled so, its peak stands drive_db above the ceiling (drive_db = 0: peak normalisation to the
    ceiling, the gain 1 throughout; there pre_gain is lowered by the ulp or two it takes for fl(pre_gain * peak) <= fl(c) in fp32) --, 1 for a silent clip (peak 0); W = lookahead_samples(rate, lookahead_seconds)."""
    ceiling_db, drive_db, peak = _number("ceiling_db", ceiling_db), _number("drive_db", drive_db), _number("peak", peak)
    if ceiling_db > 0:
        raise ValueError(f"limiter: ceiling_db must not be above 0 dBFS (got {ceiling_db})")
    if drive_db < 0:
        raise ValueError(f"limiter: drive_db must not be negative (got {drive_db})")
    if peak < 0:
        raise ValueError(f"limiter: peak must not be negative (got {peak})")
    w = lookahead_samples(rate, lookahead_seconds)
    c = 10.0 ** (ceiling_db / 20.0)
    pre_gain = c * 10.0 ** (drive_db / 20.0) / peak if peak > 0 else 1.0
    if drive_db == 0 and peak > 0:   # the fp32 numbers the kernel multiplies: the scaled peak must not round past the ceiling by an ulp
        p32, c32, peak32 = np.float32(pre_gain), np.float32(c), np.float32(peak)
        while p32 > 0 and np.float32(p32 * peak32) > c32:
            p32 = np.nextafter(p32, np.float32(0))
        if p32 != np.float32(pre_gain):
            pre_gain = float(p32)
    return pre_gain, c, w


def apply(clip, rate, ceiling_db=-1.0, drive_db=6.0, lookahead_seconds=0.005, peak=None, want_pcm=False, true_peak=False):
    """The limiter on clip ([n] or [2, n] fp32 on the device) at `rate` samples per second: -> (out, pcm or None, peak [1], min_gain [1]) of
    kernels.limit with design()'s numbers.  `peak`: the unnormalised clip's max |sample| as the stage before returned it (a number or a
    one-element tensor); None: taken here.  Both channels share ONE gain.  `true_peak`: the ceiling is in dBTP -- the pre-gain is designed
    from the clip's true peak (measured here; `peak` is not used) and the detector's envelope goes to the kernel with the clip."""
    from . import kernels
    if not isinstance(clip, torch.Tensor) or clip.dim() not in (1, 2) or clip.dtype != torch.float32 or clip.numel() == 0 or \
            (clip.dim() == 2 and clip.shape[0] != 2):
        got = f"{tuple(clip.shape)} {clip.dtype}" if isinstance(clip, torch.Tensor) else type(clip).__name__
        raise ValueError(f"limiter.apply: clip must be [n] or [2, n] fp32 (got {got})")
    envelope = None
    if true_peak:
        envelope, peak = kernels.true_peak(clip, want_envelope=True)
    if peak is None:
        peak = clip.abs().max()
    if isinstance(peak, torch.Tensor):
        if peak.numel() != 1:
            raise ValueError(f"limiter.apply: peak must be one number (got a tensor of {tuple(peak.shape)})")
        peak = float(peak)
    pre_gain, c, w = design(rate, ceiling_db, drive_db, lookahead_seconds, peak)
    if envelope is None:   # (the call it was)
        return kernels.limit(clip, pre_gain, c, w, want_pcm=want_pcm)
    return kernels.limit(clip, pre_gain, c, w, want_pcm=want_pcm, envelope=envelope)
