"""The kernel inception distance of a generated feature set against a real one, on the device (metrics.kernel_inception_distance_device;
DESIGN.md "KID on the device").

KID (Binkowski et al. 2018, "Demystifying MMD GANs") is the unbiased estimate of the squared maximum mean discrepancy between two feature sets
under the cubic polynomial kernel.  Unlike the Frechet distance its expectation does not depend on the sample count -- a figure taken on 2 000
notes compares with one taken on 50 000 -- and it comes with a spread over subsets.  The rules below are this project's own statement of it, and
tests/kid_ref.py restates every one.

Let x be the real features [n, d] and y the fake ones [m, d], both fp32.

  Kernel      k(a, b) = (a.b / d + 1)^3: degree 3, gamma 1 / d, coefficient 1, the constants of the paper and of every implementation users
              compare against.
  Sums        Sxx = sum over i != j of k(x_i, x_j), Syy = sum over i != j of k(y_i, y_j), Sxy = sum over all i, j of k(x_i, y_j).  Only the index
              excludes: a duplicate row elsewhere is a pair like any other.
  Estimate    KID = Sxx / (n (n - 1)) + Syy / (m (m - 1)) - 2 Sxy / (n m), float64 on the host from the three doubles.  It may be negative: that
              is what unbiased means, and nothing clamps it.
  Full set    `kid`: the estimate over all rows of both sets.
  Subsets     `subset_mean` and `subset_std`: the mean and the population standard deviation (ddof = 0) of the estimate over `subsets` subsets of
              size = min(subset_size, n, m) rows a side (defaults 100 and 1000, the numbers other tools print).  The subsets are drawn on the host
              by rng = numpy.random.default_rng(seed): for s in order, first rng.choice(n, size, replace=False), then rng.choice(m, size,
              replace=False).  The index lists go to the device as int32; no gathered copy of the rows is made.
  Arithmetic  on the device (gs_kid_sums): the features are widened fp32 -> fp64, which is exact; the dot is accumulated in fp64 by the fp64 MFMA
              over the columns in ascending steps of 4 -- every product is exact, only the additions round; t = p / d + 1.0, then k = t t t, in
              fp64; every sum in fp64 in one fixed order, no float atomics.  Two calls with the same arguments give the same bits, and a subset's
              three sums have the same bits whether it is computed alone or as entry s of a batch.
  Refusals    a set with fewer than 2 rows, sets of different widths, size < 2, subsets < 0, an index outside its set: ValueError.

Two launches for the full sets and two for all the subsets together; no n x m array exists at any time.
"""
import collections

import numpy as np

from . import kernels

KidResult = collections.namedtuple("KidResult", "kid subset_mean subset_std subset_kids sums subset_sums size")
KidResult.__doc__ = """kid, subset_mean, subset_std (float; the last two NaN with subsets = 0); subset_kids [subsets] float64: the estimate of every
subset; sums [3] float64: Sxx, Syy, Sxy of the full sets; subset_sums [subsets, 3] float64; size: the rows a side of a subset.  The arrays are
numpy, on the host."""


def _count(what, name, v, low):
    if not isinstance(v, (int, np.integer)) or isinstance(v, bool) or v < low:
        raise ValueError(f"{what}: {name} must be an integer >= {low} (got {v!r})")
    return int(v)


def check_sets(real, fake, subsets=100, subset_size=1000, what="kid"):
    """The refusals of the module docstring for two [rows, columns] sets (anything with a shape): ValueError.  -> the rows a side of a subset."""
    for name, t in (("real", real), ("fake", fake)):
        if len(t.shape) != 2:
            raise ValueError(f"{what}: {name} must be a [rows, columns] matrix (got {tuple(t.shape)})")
        if t.shape[0] < 2:
            raise ValueError(f"{what}: {name} must have at least 2 rows (got {t.shape[0]})")
    if real.shape[1] != fake.shape[1]:
        raise ValueError(f"{what}: real and fake differ in width ({real.shape[1]} and {fake.shape[1]})")
    _count(what, "subsets", subsets, 0)
    return min(_count(what, "subset_size", subset_size, 2), int(real.shape[0]), int(fake.shape[0]))


def draw_subsets(n, m, subsets=100, subset_size=1000, seed=0):
    """The module's draws: -> (xi [subsets, size], yi [subsets, size]) int32, size = min(subset_size, n, m)."""
    n, m = _count("draw_subsets", "n", n, 2), _count("draw_subsets", "m", m, 2)
    subsets = _count("draw_subsets", "subsets", subsets, 0)
    size = min(_count("draw_subsets", "subset_size", subset_size, 2), n, m)
    rng = np.random.default_rng(seed)
    xi, yi = np.empty((subsets, size), dtype=np.int32), np.empty((subsets, size), dtype=np.int32)
    for s in range(subsets):
        xi[s] = rng.choice(n, size, replace=False)
        yi[s] = rng.choice(m, size, replace=False)
    return xi, yi


def estimate(sums, n, m):
    """KID from (Sxx, Syy, Sxy) ([..., 3], float64) of sets of n and m rows: -> float64 of shape [...]."""
    n, m = _count("estimate", "n", n, 2), _count("estimate", "m", m, 2)
    sums = np.asarray(sums, dtype=np.float64)
    if sums.shape[-1:] != (3,):
        raise ValueError(f"estimate: sums must end in the three sums Sxx, Syy, Sxy (got {sums.shape})")
    return sums[..., 0] / (n * (n - 1)) + sums[..., 1] / (m * (m - 1)) - 2.0 * sums[..., 2] / (n * m)


def figures(real, fake, subsets=100, subset_size=1000, seed=0):
    """The module's rules on real [n, d] and fake [m, d] (fp32 on the device): -> KidResult."""
    size = check_sets(real, fake, subsets, subset_size)
    n, m = int(real.shape[0]), int(fake.shape[0])
    sums = kernels.kid_sums(real, fake).cpu().numpy()[0]
    if subsets:
        xi, yi = draw_subsets(n, m, subsets, subset_size, seed)
        subset_sums = kernels.kid_sums(real, fake, xi, yi).cpu().numpy()
        subset_kids = estimate(subset_sums, size, size)
        mean, std = float(subset_kids.mean()), float(subset_kids.std())
    else:
        subset_sums, subset_kids, mean, std = np.zeros((0, 3)), np.zeros((0,)), float("nan"), float("nan")
    return KidResult(kid=float(estimate(sums, n, m)), subset_mean=mean, subset_std=std, subset_kids=subset_kids, sums=sums, subset_sums=subset_sums, size=size)
