"""A float64 numpy restatement of the rules of gansynth_amd/pitch.py and of gs_yin_difference / gs_yin_pick / gs_yin_track
(include/gansynth_hip.h; DESIGN.md "Pitch tracking on the device"): a direct transcription, built on nothing of the package but the synthetic
notes of dataset.synthetic_nsynth_input_fn.  The difference function comes from per-lag cumulative sums; everything else is the rule as written.

  frames(n, W, L, hop)               F = (n - W - L) // hop + 1
  difference(x, W, L, hop)           rule 1 for one row: d [F, L] and power [F]
  normalise(d)                       rule 2: c [F, L], the sum sequential and ascending (np.cumsum)
  pick(d, tau_min, threshold)        rules 2-4 on d [F, L]: lag, period, aperiodicity and, per frame, whether any comparison made on the way had
                                     its two sides within NEAR, relative, of each other without being equal (`ambiguous`)
  track(x, ...)                      pick(difference(x)) and the power
  note(period, aper, power, pitch)   rule 5 for one note: (median cents, jitter, voiced frames)
  synthetic_note(pitch)              one note exactly as dataset.synthetic_nsynth_input_fn makes it (seed 0)
  harmonic_rows(rows, n, seed)       the kernels' test signals: seeded harmonic notes plus 0.002 noise, one row of noise, one of zeros"""
import functools

import numpy as np

U = 2.0 ** -24
RATE, WINDOW, LAGS, HOP, TAU_MIN, THRESHOLD = 16000, 1024, 512, 256, 8, 0.15
POWER_GATE = 1.0e-4
NEAR = 1.0e-12


def dist_bound(W):
    """kmeans_ref.dist_bound(W): a fp32 sum of W non-negative rounded squares of rounded differences, in any order -- relative."""
    return (W + 8) * U


def frames(n, W, L, hop):
    return (n - W - L) // hop + 1


def difference(x, W, L, hop):
    """One row x [n] -> (d [F, L], power [F]) in float64: d(f, tau) = sum_{j < W} (x[t + j] - x[t + j + tau])^2, t = f hop, as the difference of
    a cumulative sum per lag."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    F = frames(n, W, L, hop)
    t = np.arange(F) * hop
    d = np.zeros((F, L))
    g = int(np.gcd(hop, W))                             # every frame starts and ends on a multiple of g: the cumulative sum runs over blocks of g
    m = ((F - 1) * hop + W) // g
    lo, hi = t // g, (t + W) // g

    def window_sums(e):                                 # sum of e[t .. t + W) for every frame
        cs = np.concatenate([[0.0], np.cumsum(e.reshape(m, g).sum(axis=1))])
        return cs[hi] - cs[lo]

    for tau in range(1, L):
        e = x[:m * g] - x[tau:tau + m * g]
        e *= e
        d[:, tau] = window_sums(e)
    return d, window_sums(x[:m * g] ** 2) / W


def normalise(d):
    d = np.asarray(d, dtype=np.float64)
    S = np.cumsum(d[:, 1:], axis=1)                     # sequential, ascending
    c = np.ones_like(d)
    tau = np.arange(1, d.shape[1], dtype=np.float64)[None, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        c[:, 1:] = np.where(S == 0.0, 1.0, d[:, 1:] * tau / S)
    return c


def _near(a, b):
    return a != b and abs(a - b) <= NEAR * max(abs(a), abs(b))


def pick(d, tau_min=TAU_MIN, threshold=THRESHOLD):
    """d [F, L] -> (lag [F] int, period [F], aperiodicity [F], ambiguous [F] bool)."""
    c = normalise(d)
    F, L = c.shape
    hi = L - 2
    lag, period, aper, ambiguous = np.zeros(F, dtype=np.int64), np.zeros(F), np.zeros(F), np.zeros(F, dtype=bool)
    for f in range(F):
        row = c[f]
        amb = False
        below = np.nonzero(row[tau_min:hi + 1] < threshold)[0]
        if below.size:
            tau = tau_min + int(below[0])
            amb |= bool((np.abs(row[tau_min:tau + 1] - threshold) <= NEAR * np.maximum(np.abs(row[tau_min:tau + 1]), threshold)).any())
            while tau + 1 <= hi:
                amb |= _near(row[tau + 1], row[tau])
                if not row[tau + 1] < row[tau]:
                    break
                tau += 1
        else:
            seg = row[tau_min:hi + 1]
            amb |= bool((np.abs(seg - threshold) <= NEAR * np.maximum(np.abs(seg), threshold)).any())
            tau = tau_min + int(np.argmin(seg))          # (the lowest index on a tie)
            best = row[tau]
            amb |= bool(((seg != best) & (np.abs(seg - best) <= NEAR * np.maximum(np.abs(seg), abs(best)))).any())
        cm, c0, cp = row[tau - 1], row[tau], row[tau + 1]
        den = cm - 2.0 * c0 + cp
        amb |= den != 0.0 and abs(den) <= NEAR * max(abs(cm), abs(2.0 * c0), abs(cp))
        off = 0.0
        if den > 0.0:
            off = 0.5 * (cm - cp) / den
            amb |= _near(abs(off), 1.0)
            off = min(1.0, max(-1.0, off))
        lag[f], period[f], aper[f], ambiguous[f] = tau, tau + off, c0, amb
    return lag, period, aper, ambiguous


def track(x, W=WINDOW, L=LAGS, hop=HOP, tau_min=TAU_MIN, threshold=THRESHOLD):
    """One row -> (lag, period, aperiodicity, power), all float64 rules."""
    d, power = difference(x, W, L, hop)
    lag, period, aper, _ = pick(d, tau_min, threshold)
    return lag, period, aper, power


def label_frequency(pitch):
    return 440.0 * 2.0 ** ((float(pitch) - 69.0) / 12.0)


def note(period, aper, power, pitch, rate=RATE, threshold=THRESHOLD):
    """Rule 5 for one note: -> (median cents, jitter, voiced frames); NaN, NaN, 0 for an unvoiced note."""
    period, aper, power = (np.asarray(a, dtype=np.float64) for a in (period, aper, power))
    voiced = (aper < threshold) & (power > POWER_GATE * power.max())
    if not voiced.any():
        return float("nan"), float("nan"), 0
    cents = 1200.0 * np.log2((rate / period[voiced]) / label_frequency(pitch))
    return float(np.median(cents)), float(np.std(cents)), int(voiced.sum())


@functools.lru_cache(maxsize=None)
def synthetic_note(pitch):
    """One note of `pitch` [64000] fp32, read-only: the first note of dataset.synthetic_nsynth_input_fn(1, pitches=[pitch], seed=0)."""
    from gansynth_amd import dataset
    wav, lab = dataset.synthetic_nsynth_input_fn(1, pitches=[pitch], num_batches=1, seed=0)()
    assert wav.shape == (1, 64000) and lab.shape == (1, 1)
    out = wav[0].numpy().copy()
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def synthetic_tracks(pitch):
    """(d [245, 512], power [245]) of synthetic_note(pitch) at the production parameters, float64, read-only."""
    d, power = difference(synthetic_note(pitch), WINDOW, LAGS, HOP)
    d.setflags(write=False)
    power.setflags(write=False)
    return d, power


def harmonic_rows(rows, n, seed):
    """[rows, n] fp32: seeded harmonic notes (four harmonics, a period between 20 and 200 samples, peak 0.5) plus 0.002 noise; with three rows
    or more the last but one is pure noise and the last all zeros; with two the last is noise."""
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64)
    x = np.zeros((rows, n))
    for r in range(rows):
        period = rng.uniform(20.0, 200.0)
        for h in range(1, 5):
            x[r] += rng.uniform(0.2, 1.0) / h * np.sin(2.0 * np.pi * h * t / period + rng.uniform(0.0, 2.0 * np.pi))
        x[r] = 0.5 * x[r] / np.abs(x[r]).max() + rng.normal(0.0, 0.002, n)
    if rows >= 2:
        x[rows - 2 if rows >= 3 else rows - 1] = rng.normal(0.0, 0.3, n)
    if rows >= 3:
        x[rows - 1] = 0.0
    return x.astype(np.float32)
