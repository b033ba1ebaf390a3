"""The loudness meter's rule (include/gansynth_hip.h, DESIGN.md "Loudness") restated in numpy -- what gs_loudness and gansynth_amd/loudness.py
are held to.

    coefficients(rate)      the two K-weighting sections by the bilinear forms, float64 (numpy's tan and power, not the library's)
    energy_f64(x, rate)     the rule in float64: scipy.signal.lfilter cascade from rest, squares, hop sums -> [rows, hops]
    energy_f32(x, rate)     a sequential fp32 restatement: transposed direct form II, one rounding per operation, no FMA; squares and a
                            running hop sum in fp32
    integrated(energy, hop) BS.1770-4 gating in float64
    chunked_f64(x, design)  the library's chunking restated (the lanes' ends from rest, the two scans with the descriptor's matrix powers,
                            the second run): shows on the CPU that the descriptor's matrices carry the states the sequential filter has
The error of hop energies z against energy_f64's z64 is e(z) = max |z - z64| / max z64 over all rows and hops -- a per-hop relative error
means nothing in a silent hop -- and a kernel is bounded by FACTOR times energy_f32's e on the same input: the project's margin for a kernel
against a float restatement (tests/limiter_ref.py, tests/reverb_ref.py), not tuned to this kernel.
The inputs of the GPU tests are prefixes of ONE master signal per (rate, kind), two seconds long, so that both restatements run once per
rate and every length reads its hops from them (a causal filter: the hops of a prefix are a prefix of the hops)."""
import functools

import numpy as np
from scipy import signal

FACTOR = 4.0
NT = 256                      # lanes of a block of gs_loudness
RATES = (16000, 44100, 48000)
KINDS = ("dc_noise", "constant", "silence_burst", "seam_steps")
SECONDS = 2
# ITU-R BS.1770-4, table 1 and 2 (48 kHz)
TABLE_48K = (((1.53512485958697, -2.69169618940638, 1.19839281085285), (1.0, -1.69065929318241, 0.73248077421585)),
             ((1.0, -2.0, 1.0), (1.0, -1.99004745483398, 0.99007225036621)))


def hop_of(rate):
    return int(np.floor(0.1 * rate + 0.5))


def coefficients(rate):
    """-> ((b1, a1), (b2, a2)) float64, a[0] = 1."""
    def section(f0, q, shelf):
        k = np.tan(np.pi * f0 / rate)
        a0 = 1.0 + k / q + k * k
        if shelf:
            vh = 10.0 ** (3.999843853973347 / 20.0)
            vb = vh ** 0.4996667741545416
            b = np.array([vh + vb * k / q + k * k, 2.0 * (k * k - vh), vh - vb * k / q + k * k]) / a0
        else:
            b = np.array([1.0, -2.0, 1.0])
        return b, np.array([1.0, 2.0 * (k * k - 1.0) / a0, (1.0 - k / q + k * k) / a0])
    return section(1681.974450955533, 0.7071752369554196, True), section(38.13547087602444, 0.5003270373238773, False)


def k_weighted_f64(x, rate):
    (b1, a1), (b2, a2) = coefficients(rate)
    x = np.atleast_2d(np.asarray(x)).astype(np.float64)
    return signal.lfilter(b2, a2, signal.lfilter(b1, a1, x, axis=-1), axis=-1)


def hop_sums(y, hop):
    y = np.atleast_2d(y)
    hops = y.shape[1] // hop
    return (y[:, :hops * hop].reshape(y.shape[0], hops, hop) ** 2).sum(axis=2)


def energy_f64(x, rate):
    return hop_sums(k_weighted_f64(x, rate), hop_of(rate))


def energy_f32(x, rate):
    """Sample after sample in fp32 (vectorised over the rows only): every product and every sum rounded on its own."""
    (b1, a1), (b2, a2) = coefficients(rate)
    f = np.float32
    b10, b11, b12, a11, a12 = f(b1[0]), f(b1[1]), f(b1[2]), f(a1[1]), f(a1[2])
    b20, b21, b22, a21, a22 = f(b2[0]), f(b2[1]), f(b2[2]), f(a2[1]), f(a2[2])
    x = np.atleast_2d(np.asarray(x, dtype=np.float32))
    rows, n = x.shape
    hop = hop_of(rate)
    hops = n // hop
    out = np.zeros((rows, hops), dtype=np.float32)
    s0, s1, s2, s3 = (np.zeros(rows, dtype=np.float32) for _ in range(4))
    xt = np.ascontiguousarray(x.T)
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(hops):
            acc = np.zeros(rows, dtype=np.float32)
            for t in range(j * hop, (j + 1) * hop):
                v = xt[t]
                y1 = b10 * v + s0
                s0 = (b11 * v - a11 * y1) + s1
                s1 = b12 * v - a12 * y1
                y2 = b20 * y1 + s2
                s2 = (b21 * y1 - a21 * y2) + s3
                s3 = b22 * y1 - a22 * y2
                acc = acc + y2 * y2
            out[:, j] = acc
    return out


def error(z, z64):
    """e(z) of the module's docstring; 0 for no hops or an all-silent reference."""
    z, z64 = np.atleast_2d(np.asarray(z, dtype=np.float64)), np.atleast_2d(z64)
    assert z.shape == z64.shape, (z.shape, z64.shape)
    top = z64.max() if z64.size else 0.0
    return float(np.abs(z - z64).max() / top) if top > 0 else float(np.abs(z).max() if z.size else 0.0)


# ------------------------------------------------------------------------------------------------------------------ gating
def block_loudness(energy, hop):
    e = np.atleast_2d(np.asarray(energy, dtype=np.float64))
    if e.shape[1] < 4:
        return np.empty(0)
    z = sum(e[:, k:e.shape[1] - 3 + k] for k in range(4)).sum(axis=0) / (4.0 * hop)
    with np.errstate(divide="ignore"):
        return -0.691 + 10.0 * np.log10(z)


def _gates(energy, hop):
    l = block_loudness(energy, hop)
    above = l > -70.0
    if not above.any():
        return l, above, None
    z = 10.0 ** ((l + 0.691) / 10.0)
    return l, above, -0.691 + 10.0 * np.log10(z[above].mean()) - 10.0


def integrated(energy, hop):
    l, above, gate = _gates(energy, hop)
    if gate is None:
        return -np.inf
    z = 10.0 ** ((l + 0.691) / 10.0)
    return float(-0.691 + 10.0 * np.log10(z[above & (l > gate)].mean()))


def gate_margin(energy, hop):
    """The distance in LU of the nearest gating block to either gate (inf when there is no block, or none above the absolute gate and none
    near it)."""
    l, above, gate = _gates(energy, hop)
    l = l[np.isfinite(l)]
    if l.size == 0:
        return np.inf
    d = np.abs(l + 70.0).min()
    return float(d if gate is None else min(d, np.abs(l - gate).min()))


def lufs_of(x, rate):
    return integrated(energy_f64(x, rate), hop_of(rate))


# ------------------------------------------------------------------------------------------------------------------ the GPU cases
def lengths(rate):
    """The clip lengths of the issue; the kernel's tile T is a hop."""
    hop = T = hop_of(rate)
    return sorted({hop - 1, hop, hop + 1, 4 * hop, 4 * hop + 1, T - 1, T, T + 1, 3 * T + 5, SECONDS * rate})


@functools.lru_cache(maxsize=None)
def master(rate, kind):
    """[2, SECONDS * rate] fp32, read-only; row 1 is another draw (or another level), never a copy of row 0."""
    n, hop = SECONDS * rate, hop_of(rate)
    g = np.random.Generator(np.random.PCG64(rate * 31 + KINDS.index(kind)))
    if kind == "dc_noise":        # the high-pass state is large: it must be carried exactly
        x = (g.uniform(-0.25, 0.25, (2, n)) + np.array([[0.6], [-0.45]])).astype(np.float32)
    elif kind == "constant":      # later hops decay towards 0
        x = np.stack([np.full(n, 1.0), np.full(n, -0.5)]).astype(np.float32)
    elif kind == "silence_burst":  # a second of exact zeros, then noise; row 1 wakes up a hop and three samples later
        x = np.zeros((2, n), dtype=np.float32)
        x[0, rate:] = g.uniform(-0.8, 0.8, n - rate)
        x[1, rate + hop + 3:] = g.uniform(-0.5, 0.5, n - rate - hop - 3)
    else:                         # a step on each side of every tile seam: at seam - 1, seam, seam + 1 in turn (row 1 a seam later in the turn)
        x = np.zeros((2, n), dtype=np.float32)
        for r in range(2):
            level, at = 0.0, 0
            for j, seam in enumerate(range(hop, n, hop)):
                step = seam + (j + r) % 3 - 1
                x[r, at:step] = level
                level, at = (0.7 if j % 2 == 0 else -0.3) * (1 - 0.4 * r), step
            x[r, at:] = level
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def master_energies(rate):
    """{kind: (z64 [2, hops], z32 [2, hops])} of the master signals of one rate, read-only: both restatements run once, over all kinds."""
    x = np.concatenate([master(rate, kind) for kind in KINDS])
    z64, z32 = energy_f64(x, rate), energy_f32(x, rate)
    z64.setflags(write=False)
    z32.setflags(write=False)
    return {kind: (z64[2 * i:2 * i + 2], z32[2 * i:2 * i + 2]) for i, kind in enumerate(KINDS)}


# ------------------------------------------------------------------------------------------------------------------ the chunking, restated
def _run(coef, x, s):
    """x [..., k] through both sections from the states s [..., 4] (float64): -> (sum of squares [...], end states)."""
    (b1, a1), (b2, a2) = coef
    s = [s[..., c].copy() for c in range(4)]
    acc = np.zeros(x.shape[:-1])
    for t in range(x.shape[-1]):
        v = x[..., t]
        y1 = b1[0] * v + s[0]
        s[0] = b1[1] * v - a1[1] * y1 + s[1]
        s[1] = b1[2] * v - a1[2] * y1
        y2 = b2[0] * y1 + s[2]
        s[2] = b2[1] * y1 - a2[1] * y2 + s[3]
        s[3] = b2[2] * y1 - a2[2] * y2
        acc = acc + y2 * y2
    return acc, np.stack(s, axis=-1)


def _scan(v, powers):
    """Hillis-Steele along axis -2 of v [..., NT, 4] with the matrices powers[k] = P^(2^k)."""
    v = v.copy()
    for k in range(len(powers)):
        d = 1 << k
        moved = np.einsum("rc,...c->...r", powers[k], v[..., :-d, :])
        v[..., d:, :] = v[..., d:, :] + moved
    return v


def chunked_f64(x, coef, hop, chunk, chunk_pow, hop_pow, rem_pow):
    """One row x [n] as gs_loudness's three launches treat it, in float64: -> energies [hops]."""
    hops = len(x) // hop
    last = (hop + chunk - 1) // chunk - 1
    rem = hop - last * chunk
    xs = np.asarray(x[:hops * hop], dtype=np.float64).reshape(hops, hop)
    whole = xs[:, :last * chunk].reshape(hops, last, chunk)
    tail = xs[:, last * chunk:]
    rest = np.zeros((hops, last, 4))
    z = _run(coef, whole, rest)[1]                                  # the whole chunks' ends from rest
    z_tail = _run(coef, tail, np.zeros((hops, 4)))[1]

    def starts(seed):                                               # [hops, 4] -> the state every lane's chunk starts in [hops, last + 1, 4]
        v = np.zeros((hops, NT, 4))
        v[:, :last] = z
        if last > 0:
            v[:, 0] += seed @ chunk_pow[0].T
        v = _scan(v, chunk_pow)
        return np.concatenate([seed[:, None, :], v[:, :last]], axis=1)

    ends = starts(np.zeros((hops, 4)))[:, last] @ rem_pow.T + z_tail   # launch 1: Z
    S = np.zeros((hops, 4))                                            # launch 2
    carry = np.zeros(4)
    for t0 in range(0, hops, NT):
        v = np.zeros((NT, 4))
        v[:min(NT, hops - t0)] = ends[t0:t0 + NT]
        S[t0] = carry
        v[0] += hop_pow[0] @ carry
        v = _scan(v, hop_pow)
        m = min(NT - 1, hops - t0 - 1)
        S[t0 + 1:t0 + 1 + m] = v[:m]
        carry = v[NT - 1]
    st = starts(S)                                                     # launch 3
    return _run(coef, whole, st[:, :last])[0].sum(axis=1) + _run(coef, tail, st[:, last])[0]
