"""The rules of gansynth_amd/swd.py restated in float64 numpy (include/gansynth_hip.h, DESIGN.md "SWD on the device"), and the bounds the SWD tests
hold the kernels to.  Nothing here imports the package.  u = 2^-24 (fp32 unit roundoff), gamma(k) = k u / (1 - k u)."""
import functools

import numpy as np

U = 2.0 ** -24
PATCHES, PATCH, DESC, REPEATS, DIRECTIONS = 128, 7, 98, 4, 128
SORT_TILE, MAX_N, MAX_ROWS, MAX_SIDE, MAX_BATCH = 4096, 1 << 21, 65535, 16384, 65536
K5 = np.array([1.0, 4.0, 6.0, 4.0, 1.0])


def gamma(k):
    return k * U / (1.0 - k * U)


def levels(h, w):
    """The number of l >= 0 with min(h, w) >> l >= 16; 0 (refused) without one, with an odd size that is halved, or past MAX_SIDE."""
    if min(h, w) < 16 or max(h, w) > MAX_SIDE:
        return 0
    count = 0
    while min(h, w) >= 16:
        count += 1
        if min(h, w) // 2 < 16:
            break
        if h % 2 or w % 2:
            return 0
        h, w = h // 2, w // 2
    return count if min(h, w) >= 7 else 0


def _filter(x, gain):
    """x [..., H, W] filtered by gain * outer(K5, K5) / 256, the border mirrored without the edge sample (numpy's "reflect")."""
    pad = np.pad(x, [(0, 0)] * (x.ndim - 2) + [(2, 2), (2, 2)], mode="reflect")
    h, w = x.shape[-2:]
    out = np.zeros_like(x)
    for dy in range(5):
        for dx in range(5):
            out += (gain * K5[dy] * K5[dx] / 256.0) * pad[..., dy:dy + h, dx:dx + w]
    return out


def down(g):
    return _filter(g, 1.0)[..., ::2, ::2]


def up(g):
    z = np.zeros(g.shape[:-2] + (2 * g.shape[-2], 2 * g.shape[-1]), dtype=g.dtype)
    z[..., ::2, ::2] = g
    return _filter(z, 4.0)


def laplacian(x):
    """x [n, 2, h, w] -> its Laplacian levels (float64), finest first."""
    g = [np.asarray(x, dtype=np.float64)]
    for _ in range(1, levels(*x.shape[-2:])):
        g.append(down(g[-1]))
    return [g[l] - up(g[l + 1]) for l in range(len(g) - 1)] + [g[-1]]


def reconstruct(laps):
    x = laps[-1]
    for lap in laps[-2::-1]:
        x = lap + up(x)
    return x


def corners(seed, batches, h, w):
    """The corner stream of one set: for every batch size of `batches`, in order, per level ascending integers(0, h_l - 6, (b, 128)) then
    integers(0, w_l - 6, (b, 128)).  -> per level (ys, xs) of all images, [n, 128] each."""
    rng = np.random.Generator(np.random.PCG64(seed))
    count = levels(h, w)
    ys, xs = [[] for _ in range(count)], [[] for _ in range(count)]
    for b in batches:
        for l in range(count):
            ys[l].append(rng.integers(0, (h >> l) - 6, (b, PATCHES)))
            xs[l].append(rng.integers(0, (w >> l) - 6, (b, PATCHES)))
    return [(np.concatenate(ys[l]), np.concatenate(xs[l])) for l in range(count)]


def directions(seed):
    rng = np.random.Generator(np.random.PCG64(seed + 2))
    out = []
    for _ in range(REPEATS):
        d = rng.standard_normal((DESC, DIRECTIONS))
        out.append((d / np.sqrt((d ** 2).sum(axis=0))).astype(np.float32))
    return np.concatenate(out, axis=1)


def descriptors(level, ys, xs):
    """level [n, 2, h, w], ys / xs [n, 128] -> [n * 128, 98], index (c * 7 + dy) * 7 + dx: plain numpy indexing."""
    n = level.shape[0]
    i = np.arange(n)[:, None, None, None, None]
    c = np.arange(2)[None, None, :, None, None]
    yy = ys[:, :, None, None, None] + np.arange(PATCH)[None, None, None, :, None]
    xx = xs[:, :, None, None, None] + np.arange(PATCH)[None, None, None, None, :]
    return level[i, c, yy, xx].reshape(n * PATCHES, DESC)


def channel_moments(desc):
    """-> (mean [2], population std [2]) of the two channels of desc [rows, 98], in float64."""
    d = np.asarray(desc, dtype=np.float64).reshape(-1, 2, 49)
    return d.mean(axis=(0, 2)), d.std(axis=(0, 2))


def normalise(desc, mean, std):
    d = np.asarray(desc, dtype=np.float64).reshape(-1, 2, 49)
    return ((d - np.asarray(mean, dtype=np.float64)[None, :, None]) / np.asarray(std, dtype=np.float64)[None, :, None]).reshape(-1, DESC)


def swd(real, fake, seed=0, batch_size=None, same_corners=False):
    """The whole metric in float64.  -> dict(levels, mean, and per level and set what the error bound is composed from: max |x|, the
    channels' mean and std, A = the largest sum_k |a_k| |d_k| of a projection, S1 = the largest sum_k |d_k| of a direction)."""
    real, fake = np.asarray(real, dtype=np.float64), np.asarray(fake, dtype=np.float64)
    n, _, h, w = real.shape
    step = n if batch_size is None else batch_size
    batches = [min(step, n - at) for at in range(0, n, step)]
    d = directions(seed).astype(np.float64)
    values, parts = [], []
    pyramids = [laplacian(real), laplacian(fake)]
    picks = [corners(seed, batches, h, w), corners(seed if same_corners else seed + 1, batches, h, w)]
    for l in range(levels(h, w)):
        proj, part = [], []
        for s in (0, 1):
            desc = descriptors(pyramids[s][l], *picks[s][l])
            mean, std = channel_moments(desc)
            if not (std > 0).all():
                raise ValueError("a channel of standard deviation 0")
            a = normalise(desc, mean, std)
            proj.append(np.sort(a @ d, axis=0))
            part.append(dict(mean=mean, std=std, A=float((np.abs(a) @ np.abs(d)).max()), S1=float(np.abs(d).sum(axis=0).max()),
                             mean_abs=float(np.abs(desc).mean()), mean_sq=float((desc ** 2).mean()), m=desc.shape[0] * 49))
        values.append(float(np.abs(proj[0] - proj[1]).mean() * 1e3))
        parts.append(part)
    return dict(levels=values, mean=float(np.mean(values)), parts=parts, sizes=[f"{h >> l}x{w >> l}" for l in range(levels(h, w))],
                max_abs=[float(np.abs(real).max()), float(np.abs(fake).max())])


# ------------------------------------------------------------------------------------------------------------- inputs
def smooth(x, times=1):
    for _ in range(times):
        x = _filter(x, 1.0)
    return x


@functools.lru_cache(maxsize=None)
def prototype(n, h, w, seed=5):
    """Two image sets [n, 2, h, w] fp32: smoothed Gaussians; the fake set smoothed more, scaled 1.2 and shifted 0.1."""
    rng = np.random.default_rng(seed)
    real = smooth(rng.standard_normal((n, 2, h, w))).astype(np.float32)
    fake = (1.2 * smooth(rng.standard_normal((n, 2, h, w)), 2) + 0.1).astype(np.float32)
    real.setflags(write=False)
    fake.setflags(write=False)
    return real, fake


# ------------------------------------------------------------------------------------------------------------- bounds
def gaussian_error(l, m):
    """|computed G_l - G_l| for inputs of magnitude at most m.  The weights are dyadic, so every product is exact; a level is a convex
    combination of the one before, so an error E of its input arrives as at most E; what a level adds is the rounding of its sums: a row
    of five taps is four additions, gamma(4) times the sum of the terms' magnitudes (at most m + E), and the five row sums, each off by
    that much, are added the same way: (2 gamma(4) + gamma(4)^2) (m + E)."""
    err = 0.0
    for _ in range(l):
        err += (2 * gamma(4) + gamma(4) ** 2) * (m + err)
    return err


def pyramid_bound(l, count, m):
    """|computed Lap_l - Lap_l| of a pyramid of `count` levels for |x| <= m.  Lap_{count-1} = G_{count-1}: gaussian_error.  Below it: the error of
    G_l, plus that of up(G_{l+1}) -- a convex combination per phase (weights 1/8 6/8 1/8 or 4/8 4/8 an axis: the error of G_{l+1} does not grow),
    at most three taps an axis, so (2 gamma(2) + gamma(2)^2) (m + E) of summation rounding --, plus the subtraction's one rounding, u times
    a result of at most 2 m plus both errors."""
    if l == count - 1:
        return gaussian_error(l, m)
    fine, coarse = gaussian_error(l, m), gaussian_error(l + 1, m)
    upped = coarse + (2 * gamma(2) + gamma(2) ** 2) * (m + coarse)
    return fine + upped + U * (2 * m + fine + upped)


def moments_bound(m, magnitude_sum):
    """A double sum of m terms in any order: gamma_{m-1} in double, below m 2^-52 times the sum of the magnitudes."""
    return m * 2.0 ** -52 * magnitude_sum


def project_bound(abs_dot):
    """|computed - exact| of one projection, abs_dot = sum_k |a_k| |d_k| with a_k the exact (x_k - mean) / std of the fp32 mean and std the
    kernel uses.  The computed a_k carries two roundings (the subtraction, the division): relative 2 u + u^2; the 98 FMAs of the chain add
    at most gamma(98) relative to the sum of magnitudes: ((1 + u)^2 (1 + gamma(98)) - 1) <= (98 + 3) u (the second-order terms are below
    1e4 u^2 = 6e-4 u)."""
    return (DESC + 3) * U * abs_dot


def projection_error(p, part):
    """The largest |device projection - float64 projection| of one set and level whose descriptors are off by at most p (pyramid_bound),
    composed from `part` (swd's record of that set and level: mean, std, A, S1, mean_abs, mean_sq, m):
      the device's mean is off by at most p (the mean of errors of at most p) plus its double summation (moments_bound / m) plus its rounding
      to fp32, u |mean|; its standard deviation by at most p (the standard deviation is a seminorm: |std(x + e) - std(x)| <= rms(e) <= p) plus
      the double summation of sumsq / m - mean^2 (its error over 2 std) plus u std for the rounding to fp32;
      numerator x - mean: off by dn = 2 p + dm; quotient: |a' - a| <= dn / s' + |a| ds / s' with s' = std - ds, the smallest across the
      channels; over a projection: dn / s' * S1 + ds / s' * A;
      then the kernel's own rounding, project_bound of the sum of magnitudes A plus that shift."""
    mean, std = np.abs(part["mean"]).max(), part["std"].min()
    m = part["m"]
    dm = p + moments_bound(m, part["mean_abs"]) + U * (mean + p)
    var_err = moments_bound(m, part["mean_sq"]) + 2 * (mean + p) * moments_bound(m, part["mean_abs"])
    ds = p + var_err / (2 * std) + U * (part["std"].max() + p)
    low = std - ds
    shift = (2 * p + dm) / low * part["S1"] + ds / low * part["A"]
    return shift + project_bound(part["A"] + shift)


def metric_bound(ref, l):
    """|device level value - float64 level value|: sorting does not expand the sup norm and neither does the mean of absolute differences, so
    1e3 (eps_A + eps_B), eps the projection_error of a set; plus the double sum of the L1 stage, below 2^-40 relative."""
    count = len(ref["levels"])
    eps = [projection_error(pyramid_bound(l, count, ref["max_abs"][s]), ref["parts"][l][s]) for s in (0, 1)]
    return 1e3 * (eps[0] + eps[1]) + 2.0 ** -40 * ref["levels"][l]


# ------------------------------------------------------------------------------------------------------------- the kernel layer in numpy
def workspace_bytes(stage, a, b=0, c=0):
    """gs_swd_workspace_bytes restated (stages 0 .. 3: pyramid (b, h, w), moments (rows), sort (rows, n), l1 (rows, n))."""
    def round16(v):
        return (v + 15) // 16 * 16

    def blocks(count):
        return min(1024, (count + 2047) // 2048)
    if stage == 0:
        count = levels(b, c) if b > 0 and c > 0 else 0
        if not 1 <= a <= MAX_BATCH or count == 0:
            return 0
        return round16(4 * sum(a * (b >> l) * (c >> l) * 2 for l in range(1, count)) + 16)
    if stage == 1:
        return round16(blocks(a * DESC) * 32) if 1 <= a <= MAX_N else 0
    if stage in (2, 3):
        if not (1 <= a <= MAX_ROWS and 1 <= b <= MAX_N):
            return 0
        return (round16(4 * a * b) if b > SORT_TILE else 16) if stage == 2 else round16(blocks(a * b) * 8)
    return 0
