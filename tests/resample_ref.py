"""The output-rate rule (DESIGN.md "Output rates", include/gansynth_hip.h) restated in numpy float64 -- written from the rule, not from
the kernel: this module is what gs_resample_design, gs_resample_table, gs_resample and the Python layers above them are held to.

    g = gcd(rate_in, rate_out)   up = rate_out / g   down = rate_in / g   c = 0.95 * min(1, up / down)   taps = 2 * ceil(32 / c)
    h(u) = c * sinc(c u) * I0(12 * sqrt(1 - a^2)) / I0(12),  a = c u / 32,  for |a| < 1, else 0
    T[p][k] = h(p / up + taps/2 - 1 - k)
    y[j] = sum_k T[(j * down) mod up][k] * x[floor(j * down / up) - taps/2 + 1 + k],   x outside [0, n_in) = 0,   n_out = ceil(n_in * up / down)
"""
import math

import numpy as np

from tests.synth_ref import pcm16  # noqa: F401  (gs_summary_audio_s16's rule, restated there)

ZEROS, ROLLOFF, BETA = 32, 0.95, 12.0
PAIRS = [(16000, 48000), (16000, 44100), (44100, 16000), (48000, 16000), (16000, 22050)]


def design(rate_in, rate_out):
    """-> (up, down, taps)."""
    g = math.gcd(rate_in, rate_out)
    up, down = rate_out // g, rate_in // g
    c = ROLLOFF * min(1.0, up / down)
    return up, down, 2 * int(math.ceil(ZEROS / c))


def out_len(n_in, up, down):
    return -(-n_in * up // down)


def kernel(u, c):
    """h(u), float64."""
    u = np.asarray(u, dtype=np.float64)
    a = c * u / ZEROS
    inside = np.abs(a) < 1.0
    window = np.i0(BETA * np.sqrt(np.where(inside, 1.0 - a * a, 0.0))) / np.i0(BETA)
    return np.where(inside, c * np.sinc(c * u) * window, 0.0)


def table(up, down, taps):
    """T [up, taps], float64 (the library rounds it once to fp32)."""
    c = ROLLOFF * min(1.0, up / down)
    p = np.arange(up, dtype=np.float64)[:, None]
    k = np.arange(taps, dtype=np.float64)[None, :]
    return kernel(p / up + (taps // 2 - 1) - k, c)


def resample(x, tab, up, down, n_out=None, outputs=None):
    """One row x [n_in] through the table `tab` [up, taps] (float64, or the library's fp32 table: widened exactly) ->
    (y, B) at all n_out outputs, or at the indices `outputs`; B[j] = sum_k |T[p][k]| * |x[i]|.  Python integers / int64 throughout."""
    x = np.asarray(x, dtype=np.float64)
    tab = np.asarray(tab, dtype=np.float64)
    n_in, taps = x.shape[0], tab.shape[1]
    if outputs is None:
        outputs = np.arange(out_len(n_in, up, down) if n_out is None else n_out, dtype=np.int64)
    j = np.asarray(outputs, dtype=np.int64)
    y, b = np.empty(j.shape[0]), np.empty(j.shape[0])
    for lo in range(0, j.shape[0], 8192):   # (in slabs: [8192, taps] gathers)
        jd = j[lo:lo + 8192] * down
        i0, p = jd // up, jd % up
        idx = i0[:, None] - taps // 2 + 1 + np.arange(taps, dtype=np.int64)[None, :]
        ok = (idx >= 0) & (idx < n_in)
        xs = np.where(ok, x[np.clip(idx, 0, n_in - 1)], 0.0)
        y[lo:lo + 8192] = (tab[p] * xs).sum(axis=1)
        b[lo:lo + 8192] = (np.abs(tab[p]) * np.abs(xs)).sum(axis=1)
    return y, b


def bound(b, taps):
    """|got - y| <= (taps + 3) * 2^-24 * B: `taps` products and taps - 1 additions in fp32, each rounding at most 2^-24 of B to first
    order, in any order and with or without FMA, with room for the second-order terms."""
    return (taps + 3) * 2.0 ** -24 * b
