"""The look-ahead limiter's rule (include/gansynth_hip.h, DESIGN.md "Limiter") restated in numpy -- what gs_limit is held to.

    limit_f64   the rule in float64, taking the fp32 y = fl(d * x) of step 1 as given (so the branch a > c cannot flip)
    limit_f32   the algorithm in fp32 by another route than the kernel's: every window's W + 1 terms summed on their own, sequentially in
                ascending order, then divided
Both return a Result: y (fp32), r, m (m[s] at index s + W, s in [-W, n)), g, out.  The errors of a kernel are measured against limit_f64 and
bounded by FACTOR times limit_f32's on the same case: the project's margin for a float restatement (tests/reverb_ref.py), which leaves room
for a different but equally short summation order.

`window_shift` (default 0) moves the minimum's window by that many samples: the variant a test uses to show that the seam cases bite."""
import collections

import numpy as np

from tests import synth_ref as SRF

T = 4096              # GS_LIMIT_TILE
MAX_W = 2048          # GS_LIMIT_MAX_LOOKAHEAD
FACTOR = 4.0
D = np.float32(1.7)                  # pre_gain of the drawn cases
C = np.float32(10.0 ** (-1.0 / 20))  # their ceiling: -1 dBFS
LOOKAHEADS = (1, 63, 64, 65, 240, 2048)
EDGE_LOOKAHEADS = (256, 257, 1024, 1025)   # on either side of the two thresholds at which gs_limit changes its kernel (18 / 24 / 32 elements a lane)

Result = collections.namedtuple("Result", "y r m g out")


def lengths(W):
    """The clip lengths of the issue for a look-ahead W, without repeats."""
    return sorted({1, 2, W, W + 1, T - 1, T, T + 1, 3 * T + 5})


def spike_positions(n, W):
    """Where a drawn clip exceeds the ceiling: 0, n - 1, both sides of every tile seam, W and W + 1 before a seam."""
    at = {0, n - 1}
    for seam in range(T, n + 2, T):
        at |= {seam - 1, seam, seam + 1, seam - W, seam - W - 1}
    return sorted(p for p in at if 0 <= p < n)


def draws(n):
    """How many independent clips of length n make up one accuracy case.  A maximum over the few samples of a short clip is a handful of
    roundings, any of which can come out exactly 0 for either side by chance; so a short clip is drawn until about 2048 samples are in
    the measure (at most 32 times), and both the kernel's and limit_f32's maxima run over all the draws."""
    return max(1, min(32, 2048 // n))


def draw(n, rows, W, seed=None, k=0):
    """A clip [rows, n] fp32: noise whose D-fold stays below C, spikes of distinct heights above it at spike_positions, a plateau across the
    second seam (its samples equal), and -- two rows -- one spike in row 1 alone (midway through the first tile) and every other one in row 0
    alone or in both.  k: the draw's number (draws(n))."""
    g = np.random.Generator(np.random.PCG64((n * 7919 + W * 31 + rows) * 64 + k if seed is None else seed))
    x = g.uniform(-0.4, 0.4, (rows, n)).astype(np.float32)
    for k, p in enumerate(spike_positions(n, W)):
        height = np.float32((0.7 + 0.9 * g.random()) * (-1) ** k)
        x[0, p] = height
        if rows == 2 and k % 2:
            x[1, p] = np.float32(-0.8) * height
    if n > 2 * T + 40:
        x[:, 2 * T - 37:2 * T + 40] = np.float32(0.93)
    if rows == 2 and n > T // 2:
        x[1, T // 2] = np.float32(1.3)
    return x


def pre(x, d):
    """Step 1: y = fl(d * x), fp32."""
    return (np.atleast_2d(np.asarray(x, dtype=np.float32)) * np.float32(d)).astype(np.float32)


def _envelope(y):
    """Step 2: the fmaxf chain from 0 over the rows of |y| (a NaN contributes nothing)."""
    return np.fmax(np.float32(0), np.fmax.reduce(np.abs(y), axis=0))


def _sliding_min(r, W, shift=0):
    """m[s] = min of r over [max(s, 0), min(s + W, n - 1)] for s in [-W, n), at index s + W.  r <= 1 and no window is empty, so ones outside
    [0, n) do not change a minimum.  Term by term: (n + W) * (W + 1) comparisons, at most 3e7 -- plain, and exact in any order."""
    n = r.shape[0]
    pad = W + abs(shift)
    base = np.concatenate([np.ones(pad, r.dtype), r, np.ones(pad + 1, r.dtype)])      # base[pad + j] = r[j]
    out = np.full(n + W, np.inf, dtype=r.dtype)
    for k in range(W + 1):
        lo = pad - W + shift + k
        out = np.minimum(out, base[lo:lo + n + W])
    return out


def _finish(g, y, c):
    """Step 6 in the dtype of g: clamp(g * y, -c, c), a NaN stays."""
    v = g[None, :] * y.astype(g.dtype)
    if g.dtype == np.float32:
        v = v.astype(np.float32)
    return np.where(v > c, c, np.where(v < -c, -c, v)).astype(g.dtype)


def limit_f64(y, c, W, window_shift=0):
    y = np.atleast_2d(np.asarray(y, dtype=np.float32))
    c64 = np.float64(np.float32(c))
    a = _envelope(y).astype(np.float64)
    r = np.where(a > c64, c64 / np.where(a > c64, a, 1.0), 1.0)
    m = _sliding_min(r, W, window_shift)
    g = np.convolve(m, np.ones(W + 1), mode="valid") / np.float64(W + 1)     # every window summed on its own, in float64
    return Result(y, r, m, g, _finish(g, y, c64))


def limit_f32(y, c, W):
    y = np.atleast_2d(np.asarray(y, dtype=np.float32))
    c32 = np.float32(c)
    a = _envelope(y)
    r = np.where(a > c32, c32 / np.where(a > c32, a, np.float32(1)), np.float32(1)).astype(np.float32)
    m = _sliding_min(r, W)
    n = y.shape[1]
    acc = np.zeros(n, dtype=np.float32)
    for k in range(W + 1):                        # m[t - W] first: ascending, one fp32 addition a term
        acc = (acc + m[k:k + n]).astype(np.float32)
    g = (acc / np.float32(W + 1)).astype(np.float32)
    return Result(y, r, m, g, _finish(g, y, c32))


def pcm(out):
    """Step 7: [n] for one row, interleaved [n, 2] for two."""
    q = SRF.pcm16(np.atleast_2d(out))
    return q[0] if q.shape[0] == 1 else np.ascontiguousarray(q.T)


def peak(out):
    """Step 8: max |out| over the samples that are not NaN, fp32 (0 when there is none)."""
    return np.float32(np.fmax.reduce(np.abs(np.asarray(out, dtype=np.float32)).ravel(), initial=np.float32(0)))


def quiet(y, c, W):
    """Where no sample within W on either side exceeds c: the rule leaves y unchanged there, bit for bit."""
    loud = (_envelope(np.atleast_2d(y)) > np.float32(c)).astype(np.int64)
    n = loud.shape[0]
    csum = np.concatenate([[0], np.cumsum(loud)])
    t = np.arange(n)
    return csum[np.minimum(t + W + 1, n)] - csum[np.maximum(t - W, 0)] == 0


def gain_error(out, ref, c, min_gain=None):
    """max |g - g64| with g recovered through out / y where |y| >= c / 4 and |out| < c (not clamped), and -- when given -- as min_gain
    against min g64."""
    out = np.atleast_2d(np.asarray(out, dtype=np.float32)).astype(np.float64)
    y = ref.y.astype(np.float64)
    c = float(np.float32(c))
    with np.errstate(invalid="ignore", divide="ignore"):
        use = (np.abs(y) >= c / 4) & (np.abs(out) < c)
        rec = np.where(use, out / np.where(use, y, 1.0), 0.0)
    e = float(np.abs(rec - ref.g[None, :])[use].max()) if use.any() else 0.0
    if min_gain is not None:
        e = max(e, abs(float(min_gain) - float(ref.g.min())))
    return e


def out_error(out, ref):
    """max |out - out64| over the samples that are not NaN."""
    out = np.atleast_2d(np.asarray(out, dtype=np.float32)).astype(np.float64)
    ok = ~np.isnan(ref.y)
    return float(np.abs(out - ref.out)[ok].max()) if ok.any() else 0.0
