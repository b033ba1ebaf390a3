"""The true-peak rule (include/gansynth_hip.h, DESIGN.md "True peak") restated in numpy float64 -- written from the rule, not from the
kernel: what gs_true_peak, gs_limit_env and the Python layers above them are held to.

    T = resample_ref.table(4, 1, 68)                     the resampler's own 1 -> 4 design (the library rounds it once to fp32)
    z[r][4t + p] = sum_k T[p][k] * x[r][t - 33 + k]      x outside [0, n) = 0
    e[t] = max over rows of max(|x[r][t]|, |z[r][4t]|, ..., |z[r][4t + 3]|)
    true_peak = max_t e[t]
    limiter: tests/limiter_ref.py's rule with step 2 replaced by a[t] = max(max_r |y[r][t]|, fl(d * env[t]))
"""
import math

import numpy as np

from tests import limiter_ref as LR
from tests import resample_ref as RR

UP, DOWN, TAPS = 4, 1, 68
BEFORE = TAPS // 2 - 1     # 33 samples before t, 34 after
TILE = 2048                # GS_TRUE_PEAK_TILE


def table64():
    return RR.table(UP, DOWN, TAPS)


def table32():
    """The table as the library hands it out: rounded once to fp32 (widened again exactly)."""
    return table64().astype(np.float32).astype(np.float64)


def oversample(x, tab):
    """x [rows, n] -> (z [rows, n, 4], B [rows, n, 4]) in float64: z[r][t][p] = z[r][4t + p] of the rule, B = sum_k |T[p][k]| |x|."""
    x = np.atleast_2d(np.asarray(x)).astype(np.float64)
    tab = np.asarray(tab, dtype=np.float64)
    padded = np.concatenate([np.zeros((x.shape[0], BEFORE)), x, np.zeros((x.shape[0], TAPS - 1 - BEFORE))], axis=1)
    win = np.lib.stride_tricks.sliding_window_view(padded, TAPS, axis=1)           # win[r][t][k] = x[r][t - 33 + k]
    return win @ tab.T, np.abs(win) @ np.abs(tab).T


def detector(x, tab=None):
    """-> (e [n] float64, bound [n]): the envelope of the rule through `tab` (default: the fp32-rounded table) and, per sample, the largest
    bound among its five terms -- |x| is exact, a z term has resample_ref.bound of its B."""
    x = np.atleast_2d(np.asarray(x)).astype(np.float64)
    z, b = oversample(x, table32() if tab is None else tab)
    e = np.maximum(np.abs(x).max(axis=0), np.abs(z).max(axis=(0, 2)))
    return e, RR.bound(b, TAPS).max(axis=(0, 2))


def true_peak(x, tab=None):
    return float(detector(x, tab)[0].max())


def db(v):
    return 20.0 * math.log10(v) if v > 0 else -math.inf


def scaled_envelope(env, d):
    """fl(d * env[t]): the fp32 product step 2' takes."""
    return (np.float32(d) * np.asarray(env, dtype=np.float32)).astype(np.float32)


def _ratio(y, scaled_env, c, dtype):
    a = LR._envelope(y)
    if scaled_env is not None:
        a = np.fmax(a, np.asarray(scaled_env, dtype=np.float32))                   # (a NaN in the envelope contributes nothing)
    a, c = a.astype(dtype), dtype(np.float32(c))
    return np.where(a > c, c / np.where(a > c, a, dtype(1)), dtype(1)).astype(dtype)


def limit_f64(y, scaled_env, c, W):
    """limiter_ref.limit_f64 with step 2': y = fl(d * x) and scaled_env = fl(d * env) are taken as the fp32 values given (None: the plain rule)."""
    y = np.atleast_2d(np.asarray(y, dtype=np.float32))
    r = _ratio(y, scaled_env, c, np.float64)
    m = LR._sliding_min(r, W)
    g = np.convolve(m, np.ones(W + 1), mode="valid") / np.float64(W + 1)
    return LR.Result(y, r, m, g, LR._finish(g, y, np.float64(np.float32(c))))


def limit_f32(y, scaled_env, c, W):
    """limiter_ref.limit_f32 with step 2': every window summed on its own in fp32, ascending."""
    y = np.atleast_2d(np.asarray(y, dtype=np.float32))
    r = _ratio(y, scaled_env, c, np.float32)
    m = LR._sliding_min(r, W)
    n = y.shape[1]
    acc = np.zeros(n, dtype=np.float32)
    for k in range(W + 1):
        acc = (acc + m[k:k + n]).astype(np.float32)
    g = (acc / np.float32(W + 1)).astype(np.float32)
    return LR.Result(y, r, m, g, LR._finish(g, y, np.float32(c)))


def quiet(y, scaled_env, c, W):
    """Where no a within W on either side exceeds c: the rule leaves y unchanged there, bit for bit."""
    a = LR._envelope(np.atleast_2d(y))
    if scaled_env is not None:
        a = np.fmax(a, scaled_env)
    loud = (a > np.float32(c)).astype(np.int64)
    n = loud.shape[0]
    csum = np.concatenate([[0], np.cumsum(loud)])
    t = np.arange(n)
    return csum[np.minimum(t + W + 1, n)] - csum[np.maximum(t - W, 0)] == 0


# ------------------------------------------------------------------------------------------------------------ the issue's four inputs
N = 8192
C_DB = -1.0
C = np.float32(10.0 ** (C_DB / 20))


def sine(period, phase, amplitude, n=N):
    return (amplitude * np.sin(2.0 * np.pi * np.arange(n) / period + phase))[None, :]


def inputs():
    """name -> x [rows, 8192] float64 (each exactly representable after the fp32 rounding the tests apply)."""
    t = np.arange(N)
    noise = np.random.default_rng(0).normal(size=(2, N)) * 0.6
    square = 1.5 * np.where(np.sin(2.0 * np.pi * 0.013 * t + 0.1) >= 0, 1.0, -1.0)[None, :]
    gate = ((t // 512) % 2 == 0).astype(np.float64)
    bursts = (np.random.default_rng(1).normal(size=N) * gate * 2.0)[None, :]
    return {"sine": sine(4, np.pi / 4, 2.0), "noise": noise, "square": square, "bursts": bursts}


def limited_true_peak_db(x, W, with_envelope, d=1.0, c=C):
    """dBTP over the ceiling of the float64 limiter's output on x, re-measured by the float64 detector."""
    x32 = np.atleast_2d(x).astype(np.float32)
    y = LR.pre(x32, d)
    env = scaled_envelope(detector(x32)[0], d) if with_envelope else None
    out = limit_f64(y, env, c, W).out
    return db(true_peak(out)) - db(float(np.float32(c)))
