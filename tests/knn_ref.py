"""A float64 numpy restatement of the rules of gansynth_amd/manifold.py and of gs_knn_kth / gs_knn_within (include/gansynth_hip.h), built on
kmeans_ref.sqdist and kmeans_ref.dist_bound.  Nothing here imports the package: the tests hold the package against this file.

  kth              the k smallest squared distances of every row of a to the rows of b (j != i with exclude_diagonal), ascending, +inf where
                   the candidates run out
  within           count[i] = #{j : |q_i - ref_j|^2 <= radius2[j]}; a NaN radius admits nothing
  figures          radii from kth(x, x, k, True)[:, k - 1]; precision, recall, density, coverage as manifold.py states them
  ambiguous_pairs  the pairs (i, j) whose float64 distance lies within the fp32 rounding of the radius: |d64 - r| <= dist_bound(d) * d64
"""
import numpy as np

from tests import kmeans_ref as KR


def kth(a, b, k, exclude_diagonal=False, dtype=np.float64):
    """-> [n, k] in `dtype`."""
    full = KR.sqdist(a, b, dtype)
    if exclude_diagonal:
        i = np.arange(min(full.shape))
        full[i, i] = np.inf
    full = np.sort(full, axis=1)[:, :k]
    if full.shape[1] < k:
        full = np.concatenate([full, np.full((full.shape[0], k - full.shape[1]), np.inf, dtype=dtype)], axis=1)
    return full


def within(q, ref, radius2, dtype=np.float64):
    """-> [n] int64."""
    with np.errstate(invalid="ignore"):
        return (KR.sqdist(q, ref, dtype) <= np.asarray(radius2, dtype=dtype)[None, :]).sum(axis=1).astype(np.int64)


def ambiguous_pairs(q, ref, radius2, d):
    """-> [n, m] bool: the pairs on which fp32 rounding of the distance may decide either way."""
    full = KR.sqdist(q, ref)
    with np.errstate(invalid="ignore"):
        return np.abs(full - np.asarray(radius2, dtype=np.float64)[None, :]) <= KR.dist_bound(d) * full


def figures(real, fake, k=3, dtype=np.float64):
    """-> dict(precision, recall, density, coverage, real_radii, fake_radii, fake_counts, real_counts, coverage_minima)."""
    real_radii, fake_radii = kth(real, real, k, True, dtype)[:, k - 1], kth(fake, fake, k, True, dtype)[:, k - 1]
    fake_counts, real_counts = within(fake, real, real_radii, dtype), within(real, fake, fake_radii, dtype)
    minima = kth(real, fake, 1, False, dtype)[:, 0]
    n, m = len(real_counts), len(fake_counts)
    return dict(precision=int(np.count_nonzero(fake_counts >= 1)) / m, recall=int(np.count_nonzero(real_counts >= 1)) / n,
                density=int(fake_counts.sum()) / (k * m), coverage=int(np.count_nonzero(minima <= real_radii)) / n,
                real_radii=real_radii, fake_radii=fake_radii, fake_counts=fake_counts, real_counts=real_counts, coverage_minima=minima)


def slices(n, m):
    """gs_knn_slices as include/gansynth_hip.h states it."""
    want = -(-3072 // -(-n // 256))
    rows = max(256, 64 * -(-(-(-m // want)) // 64))
    return -(-m // rows)


def workspace_bytes(n, m, k):
    s = slices(n, m)
    return 16 if s == 1 else -(-4 * s * n * k // 16) * 16


def clustered(n, d, rng, centres=None):
    """n fp32 rows around 8 shared centres: 4 + 0.7 N(0, 1) for the centres, + 0.5 N(0, 1) for the rows.  -> (rows, centres)."""
    if centres is None:
        centres = (4.0 + 0.7 * rng.standard_normal((8, d))).astype(np.float32)
    return (centres[rng.integers(0, 8, n)] + 0.5 * rng.standard_normal((n, d))).astype(np.float32), centres
