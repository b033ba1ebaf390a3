"""Reverb for rendered clips (not in the reference; the rules are this project's own, DESIGN.md "Reverb").

The stage sits between the resampler and the ONE peak normalisation of a rendered score: mix -> resample -> reverb -> peak -> PCM.  A tail
changes the peak, so a clip that were normalised first and reverberated afterwards would clip.

Host code, except `apply`'s call into kernels.fft_convolve (gs_fftconv: partitioned FFT convolution on the device) and `read_impulse`'s
use of spectral_ops.resample for a file at another rate.

    design_impulse(rate, rt60, channels, seed, predelay)   a room by rule: decaying Gaussian noise, -60 dB at rt60
    read_impulse(path, rate, predelay)                     a recorded room from a WAV file
    apply(clip, impulse, mix)                              (1 - mix) * clip + mix * (impulse convolved with clip), one peak, PCM
"""
import math

import numpy as np
import torch

from . import _lib

MAX_TAPS = _lib.FFTCONV_MAX_TAPS


def _predelay_samples(rate, predelay):
    if not (isinstance(rate, (int, np.integer)) and not isinstance(rate, bool)) or rate <= 0:
        raise ValueError(f"reverb: rate must be a positive integer (got {rate!r})")
    if not isinstance(predelay, (int, float)) or isinstance(predelay, bool) or not math.isfinite(predelay) or predelay < 0:
        raise ValueError(f"reverb: predelay must be a non-negative number of seconds (got {predelay!r})")
    return int(math.floor(predelay * rate + 0.5))


def _scaled(h):
    """All channels of h (float64 [channels, m]) by the ONE factor 1 / max_c ||h_c||_2, rounded once to fp32: the loudest channel has unit
    energy and the balance between the channels stays."""
    top = np.sqrt((h * h).sum(axis=1)).max()
    if not top > 0:
        raise ValueError("reverb: the impulse response is all zero")
    return torch.from_numpy((h / top).astype(np.float32))


def design_impulse(rate, rt60, channels=1, seed=0, predelay=0.0):
    """A designed room at `rate` samples per second: -> [channels, m] fp32 (host), m = pre + L with pre = floor(predelay * rate + 0.5) and
    L = ceil(rt60 * rate).  g = numpy.random.Generator(numpy.random.PCG64(seed)).standard_normal((channels, L)) in float64 -- a generator
    of its own: no global stream is touched --, h[c][pre + k] = g[c][k] * 10 ** (-3 k / (rt60 * rate)) (-60 dB at rt60), 0 before pre;
    all channels scaled by the one factor 1 / max_c ||h_c||_2 and rounded once to fp32."""
    pre = _predelay_samples(rate, predelay)
    if not isinstance(rt60, (int, float)) or isinstance(rt60, bool) or not math.isfinite(rt60) or rt60 <= 0:
        raise ValueError(f"design_impulse: rt60 must be a positive number of seconds (got {rt60!r})")
    if channels not in (1, 2):
        raise ValueError(f"design_impulse: channels must be 1 or 2 (got {channels!r})")
    length = int(math.ceil(rt60 * rate))
    if pre + length > MAX_TAPS:
        raise ValueError(f"design_impulse: rt60 {rt60} s and predelay {predelay} s at {rate} Hz are m = {pre + length} taps, more than {MAX_TAPS}")
    g = np.random.Generator(np.random.PCG64(seed)).standard_normal((channels, length))
    h = np.zeros((channels, pre + length))
    h[:, pre:] = g * 10.0 ** (-3.0 * np.arange(length) / (rt60 * rate))
    return _scaled(h)


def read_impulse(path, rate, predelay=0.0):
    """A recorded room: the mono or stereo WAV file `path` (16-bit or 32-bit integers, or floats) as [channels, m] fp32 (host) at `rate`.
    A file at another rate is brought there by spectral_ops.resample (on the device); `predelay` seconds of zeros go in front; the same
    one-factor scaling as design_impulse."""
    from scipy.io import wavfile
    pre = _predelay_samples(rate, predelay)
    file_rate, data = wavfile.read(path)
    if data.dtype == np.int16:
        data = data.astype(np.float64) / 32768.0
    elif data.dtype == np.int32:
        data = data.astype(np.float64) / 2147483648.0
    elif data.dtype in (np.float32, np.float64):
        data = data.astype(np.float64)
    else:
        raise ValueError(f"read_impulse: path {path}: samples of type {data.dtype} (16-bit or 32-bit integers or floats are read)")
    h = data[None] if data.ndim == 1 else np.ascontiguousarray(data.T)
    if h.shape[0] > 2:
        raise ValueError(f"read_impulse: path {path} has {h.shape[0]} channels (mono or stereo is read)")
    if h.shape[1] == 0:
        raise ValueError(f"read_impulse: path {path} holds no samples")
    if int(file_rate) != int(rate):
        from . import spectral_ops
        h = spectral_ops.resample(torch.from_numpy(h.astype(np.float32)).cuda(), int(file_rate), int(rate)).cpu().numpy().astype(np.float64)
    if pre + h.shape[1] > MAX_TAPS:
        raise ValueError(f"read_impulse: path {path} and predelay {predelay} s at {rate} Hz are m = {pre + h.shape[1]} taps, more than {MAX_TAPS}")
    return _scaled(np.concatenate([np.zeros((h.shape[0], pre)), h], axis=1))


def apply(clip, impulse, mix=0.25, normalize=True, want_pcm=False):
    """(1 - mix) * clip + mix * (impulse convolved with clip): -> (out, pcm or None, peak) of kernels.fft_convolve.  clip: [n] or [2, n]
    fp32 on the device; impulse: [m] or [channels, m] (a tensor or an array; it is brought to the clip's device -- hand over a device tensor
    to have its prepared spectrum reused from call to call).  A mono impulse on a stereo clip is shared by both channels, a stereo impulse
    on a mono clip is refused.  out is [n + m - 1] or [2, n + m - 1]: the tail is kept; ONE peak over both channels."""
    from . import kernels
    if not isinstance(mix, (int, float)) or isinstance(mix, bool) or not 0.0 <= mix <= 1.0:
        raise ValueError(f"reverb.apply: mix must be in [0, 1] (got {mix!r})")
    if not isinstance(clip, torch.Tensor) or clip.dim() not in (1, 2) or clip.dtype != torch.float32 or clip.numel() == 0 or \
            (clip.dim() == 2 and clip.shape[0] != 2):
        got = f"{tuple(clip.shape)} {clip.dtype}" if isinstance(clip, torch.Tensor) else type(clip).__name__
        raise ValueError(f"reverb.apply: clip must be [n] or [2, n] fp32 (got {got})")
    impulse = torch.as_tensor(impulse)
    if impulse.dim() not in (1, 2) or impulse.dtype != torch.float32 or impulse.numel() == 0 or (impulse.dim() == 2 and impulse.shape[0] > 2):
        raise ValueError(f"reverb.apply: impulse must be [m] or [1 or 2, m] fp32 (got {tuple(impulse.shape)} {impulse.dtype})")
    channels = 1 if impulse.dim() == 1 else int(impulse.shape[0])
    if channels == 2 and clip.dim() == 1:
        raise ValueError("reverb.apply: a stereo impulse needs a stereo clip (the clip is mono)")
    if impulse.dim() == 2 and (clip.dim() == 1 or channels == 1):
        impulse = impulse[0]                      # one row: shared
    return kernels.fft_convolve(clip, impulse.to(clip.device), 1.0 - mix, mix, normalize=normalize, want_pcm=want_pcm)
