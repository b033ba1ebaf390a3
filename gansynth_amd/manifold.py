"""Precision, recall, density and coverage of a generated feature set against a real one, on the device (metrics.precision_recall_device;
DESIGN.md "Precision and recall on the device").

The four figures come from two papers -- improved precision and recall (Kynkaanniemi et al. 2019), density and coverage (Naeem et al. 2020) --
and separate what FID mixes: precision and density fall when the generator makes bad notes, recall and coverage when it makes too few kinds.
The rules below are this project's own statement of them, and tests/knn_ref.py restates every one in float64 numpy.

  Distances   squared Euclidean, sum over the columns of (x - y)^2 in fp32 as one chain (gs_knn_kth, gs_knn_within): d(i, j) has the same bits
              in both entries and from either side, so a radius admits exactly the pairs that defined it.  Nothing here takes a square root.
  Radii       R_k(x_i) = the k-th smallest squared distance from x_i to the OTHER rows of its own set: knn_kth(x, x, k, exclude_diagonal=True)
              [:, k - 1].  The index alone excludes: a duplicate row is a neighbour at distance 0.  Default k = 3.
  Precision   mean over the fake rows j of [c_j >= 1], c_j = #{i : |f_j - r_i|^2 <= R_k(r_i)}: one knn_within(fake, real, R_real).
  Recall      the same with the two sets exchanged: one knn_within(real, fake, R_fake).
  Density     sum_j c_j / (k M), M the number of fake rows: the counts of precision, no launch of its own.
  Coverage    mean over the real rows i of [min_j |r_i - f_j|^2 <= R_k(r_i)]: the minimum from knn_kth(real, fake, 1), the comparison on the
              host in fp32.
  Refusals    either set with fewer than k + 1 rows (a row needs k others), sets of different widths: ValueError.
  Ratios      float64 quotients of integers, on the host.

Five launches and their folds; no distance matrix exists at any time.
"""
import collections

import numpy as np

from . import kernels

ManifoldResult = collections.namedtuple("ManifoldResult", "precision recall density coverage real_radii fake_radii fake_counts real_counts coverage_minima")
ManifoldResult.__doc__ = """precision, recall, density, coverage (float); real_radii [N] / fake_radii [M] fp32: the squared k-NN radii; fake_counts [M]
int32: the real balls every fake row lies in; real_counts [N] int32: the fake balls every real row lies in; coverage_minima [N] fp32: every real
row's squared distance to its nearest fake row.  The arrays are numpy, on the host."""


def check_sets(real, fake, k, what="manifold"):
    """The refusals of the module docstring for two [rows, columns] sets (anything with a shape): ValueError."""
    if not isinstance(k, (int, np.integer)) or isinstance(k, bool) or not 1 <= k <= kernels._lib.KNN_MAX_K:
        raise ValueError(f"{what}: k must be an integer in [1, {kernels._lib.KNN_MAX_K}] (got {k!r})")
    for name, t in (("real", real), ("fake", fake)):
        if len(t.shape) != 2:
            raise ValueError(f"{what}: {name} must be a [rows, columns] matrix (got {tuple(t.shape)})")
        if t.shape[0] < k + 1:
            raise ValueError(f"{what}: {name} must have at least k + 1 = {k + 1} rows (got {t.shape[0]})")
    if real.shape[1] != fake.shape[1]:
        raise ValueError(f"{what}: real and fake differ in width ({real.shape[1]} and {fake.shape[1]})")


def radii(x, k=3):
    """R_k of every row of x ([n, d] fp32 on the device): -> [n] fp32, contiguous, on the device."""
    return kernels.knn_kth(x, x, k, exclude_diagonal=True)[:, k - 1].contiguous()


def figures(real, fake, k=3):
    """The module's rules on real [N, d] and fake [M, d] (fp32 on the device): -> ManifoldResult."""
    check_sets(real, fake, k)
    k = int(k)
    real_radii, fake_radii = radii(real, k), radii(fake, k)
    fake_counts = kernels.knn_within(fake, real, real_radii).cpu().numpy()
    real_counts = kernels.knn_within(real, fake, fake_radii).cpu().numpy()
    minima = kernels.knn_kth(real, fake, 1)[:, 0].cpu().numpy()
    real_radii, fake_radii = real_radii.cpu().numpy(), fake_radii.cpu().numpy()
    n, m = len(real_counts), len(fake_counts)
    return ManifoldResult(precision=int(np.count_nonzero(fake_counts >= 1)) / m, recall=int(np.count_nonzero(real_counts >= 1)) / n,
                          density=int(fake_counts.sum(dtype=np.int64)) / (k * m), coverage=int(np.count_nonzero(minima <= real_radii)) / n,
                          real_radii=real_radii, fake_radii=fake_radii, fake_counts=fake_counts, real_counts=real_counts, coverage_minima=minima)
