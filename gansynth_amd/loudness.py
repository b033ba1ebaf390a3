"""Programme loudness of rendered clips: ITU-R BS.1770-4 integrated loudness in LUFS, and a loudness target (DESIGN.md "Loudness").

The render chain mix -> resample -> reverb -> limiter -> PCM sets every level by a peak; a listener hears loudness.  The meter here is the
one EBU R128 and the streaming services specify: K-weighting (two biquads), the mean square over 400 ms blocks that overlap by 75 %, an
absolute gate at -70 LUFS and a relative one 10 LU under the loudness of what passed the first.  The K-weighted energy of every 100 ms hop
comes from the device (kernels.loudness_energy, gs_loudness); the gating is float64 on the host -- a minute of audio is 600 numbers.

Host code, except `measure`'s and `apply`'s calls into the kernels.

    k_weighting(rate)                  -> ((b1, a1), (b2, a2), hop): the library's coefficients, float64
    integrated(energy, hop)            -> LUFS of hop energies [hops] or [channels, hops]; -inf when nothing passes the absolute gate
    measure(clip, rate)                -> LUFS of a [n] or [2, n] fp32 device clip
    apply(clip, rate, target_lufs, ..) -> (out, pcm or None, info): scaled to the target, peaks held under the ceiling by kernels.limit
"""
import ctypes
import math

import numpy as np
import torch

from . import _lib
from . import limiter

ABSOLUTE_GATE = -70.0   # LUFS
RELATIVE_GATE = -10.0   # LU under the loudness of the blocks above the absolute gate
OFFSET = -0.691         # BS.1770: cancels the K-weighting's gain at 997 Hz
BLOCK_HOPS = 4          # a gating block: 400 ms of 100 ms hops


def _design(rate):
    if not isinstance(rate, (int, np.integer)) or isinstance(rate, bool):
        raise ValueError(f"loudness: rate must be an integer number of samples per second (got {rate!r})")
    design = _lib.GsLoudness()
    try:
        _lib.check(_lib.load().gs_loudness_design(int(rate), ctypes.byref(design)), "gs_loudness_design")
    except _lib.GansynthHipError as e:
        raise ValueError(f"loudness: {e}")
    return design


def k_weighting(rate):
    """-> ((b1, a1), (b2, a2), hop): the shelf and the high-pass of BS.1770 at `rate` as float64 arrays of three (a[0] = 1) and the hop in
    samples, floor(0.1 * rate + 0.5) -- the numbers gs_loudness_design computes (include/gansynth_hip.h has the forms).  Needs no device."""
    d = _design(rate)
    return ((np.array(d.b1, dtype=np.float64), np.array(d.a1, dtype=np.float64)),
            (np.array(d.b2, dtype=np.float64), np.array(d.a2, dtype=np.float64)), int(d.hop))


def block_loudness(energy, hop):
    """-> l[j] = OFFSET + 10 log10(sum over the channels of the mean square over hops j .. j + 3), float64, -inf for a silent block; an
    empty array with fewer than 4 hops.  energy: [hops] or [channels, hops] sums of squares per hop of `hop` samples."""
    e = np.atleast_2d(np.asarray(energy, dtype=np.float64))
    if e.ndim != 2 or not isinstance(hop, (int, np.integer)) or isinstance(hop, bool) or hop <= 0:
        raise ValueError(f"loudness: energy must be [hops] or [channels, hops] and hop a positive integer (got {e.shape}, {hop!r})")
    if not np.isfinite(e).all():
        raise ValueError("loudness: the hop energies are not all finite (a NaN or an overflow in the clip)")
    if (e < 0).any():
        raise ValueError("loudness: a hop energy is negative")
    if e.shape[1] < BLOCK_HOPS:
        return np.empty(0, dtype=np.float64)
    z = (e[:, :-3] + e[:, 1:-2] + e[:, 2:-1] + e[:, 3:]).sum(axis=0) / (BLOCK_HOPS * float(hop))
    with np.errstate(divide="ignore"):
        return OFFSET + 10.0 * np.log10(z)


def integrated(energy, hop):
    """BS.1770-4 integrated loudness in LUFS of hop energies ([hops] or [channels, hops], channel weights 1): the mean square of the gating
    blocks above both gates, float64.  -inf with fewer than 4 hops or no block above -70 LUFS; ValueError on a non-finite energy."""
    l = block_loudness(energy, hop)
    z = 10.0 ** ((l - OFFSET) / 10.0)
    above = l > ABSOLUTE_GATE
    if not above.any():
        return -math.inf
    gate = OFFSET + 10.0 * math.log10(z[above].mean()) + RELATIVE_GATE
    kept = above & (l > gate)
    return OFFSET + 10.0 * math.log10(z[kept].mean())


def _checked_clip(what, clip):
    if not isinstance(clip, torch.Tensor) or clip.dim() not in (1, 2) or clip.dtype != torch.float32 or clip.numel() == 0 or \
            (clip.dim() == 2 and clip.shape[0] != 2):
        got = f"{tuple(clip.shape)} {clip.dtype}" if isinstance(clip, torch.Tensor) else type(clip).__name__
        raise ValueError(f"loudness.{what}: clip must be [n] or [2, n] fp32 (got {got})")


def measure(clip, rate):
    """Integrated loudness in LUFS of clip ([n] or [2, n] fp32 on the device) at `rate` samples per second."""
    from . import kernels
    _checked_clip("measure", clip)
    hop = k_weighting(rate)[2]
    return integrated(kernels.loudness_energy(clip, int(rate)).cpu().numpy(), hop)


def apply(clip, rate, target_lufs, ceiling_db=-1.0, lookahead_seconds=0.005, want_pcm=False, true_peak=False):
    """clip ([n] or [2, n] fp32 on the device) brought to `target_lufs`: measured, scaled by pre_gain = 10 ** ((target - measured) / 20) (1
    for a clip that measures -inf) and finished by kernels.limit at the ceiling -- where the scaled clip stays under it the limiter's gain is
    exactly 1 and the target is met; where not, the peaks are pulled back and the output falls short of it.  The output is measured once
    more.  -> (out, pcm or None, info) with info = dict(measured_lufs, pre_gain, output_lufs, peak, min_gain).  `true_peak`: the ceiling is in
    dBTP -- the clip's 4x oversampled envelope (kernels.true_peak) goes to the limiter with it."""
    from . import kernels
    _checked_clip("apply", clip)
    if not isinstance(target_lufs, (int, float, np.integer, np.floating)) or isinstance(target_lufs, bool) or not math.isfinite(target_lufs):
        raise ValueError(f"loudness.apply: target_lufs must be a finite number (got {target_lufs!r})")
    _, c, w = limiter.design(rate, ceiling_db, 0.0, lookahead_seconds, 0.0)   # the ceiling and the look-ahead; the level is not the limiter's
    measured = measure(clip, rate)
    pre_gain = 10.0 ** ((float(target_lufs) - measured) / 20.0) if math.isfinite(measured) else 1.0
    if true_peak:
        out, pcm, peak, min_gain = kernels.limit(clip, pre_gain, c, w, want_pcm=want_pcm, envelope=kernels.true_peak(clip, want_envelope=True)[0])
    else:
        out, pcm, peak, min_gain = kernels.limit(clip, pre_gain, c, w, want_pcm=want_pcm)
    info = dict(measured_lufs=measured, pre_gain=pre_gain, output_lufs=measure(out, rate), peak=float(peak), min_gain=float(min_gain))
    return out, pcm, info
