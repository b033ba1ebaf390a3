"""A restatement of the rules of gansynth_amd/kid.py and of gs_kid_sums (include/gansynth_hip.h).  Nothing here imports the package: the tests
hold the package against this file.

  sums          (Sxx or Sxy, its bound term) of two row sets, in numpy.longdouble, blocked by rows: every product of two fp32 features is exact
                there, and 64 bits of mantissa leave the additions eleven bits below float64's.  `same`: the set against itself, i != j only
                (the index alone excludes).  The bound term is sum over the same pairs of (sum_c |x_c y_c| / d + 1)^3, in float64.
  three_sums    (Sxx, Syy, Sxy) and their bound terms
  estimate      KID = Sxx / (n (n - 1)) + Syy / (m (m - 1)) - 2 Sxy / (n m), in the dtype of the sums
  draw_subsets  rng = default_rng(seed); for s in order rng.choice(n, size, replace=False), then rng.choice(m, size, replace=False)
  figures       kid, subset_mean, subset_std (ddof = 0), subset_kids, size in float64, with the longdouble sums and the bound terms behind them
  sum_bound     u (3 d + 8 + L) B, u = 2^-53: the device's distance from a sum, from counted roundings (tests/test_kid_gpu.py derives it)
"""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53
BLOCK = 64


def sums(x, y, same=False):
    """-> (S longdouble, B float64) over all pairs (i, j) of rows of x [n, d] and y [m, d]; with `same` (y is x) over i != j."""
    x, y = np.asarray(x), np.asarray(y)
    d = x.shape[1]
    xl, yl = x.astype(LD), y.astype(LD)
    xa, ya = np.abs(x.astype(np.float64)), np.abs(y.astype(np.float64))
    total, bound = LD(0), 0.0
    for at in range(0, x.shape[0], BLOCK):
        t = xl[at:at + BLOCK] @ yl.T / LD(d) + LD(1)
        k = t * t * t
        tb = xa[at:at + BLOCK] @ ya.T / d + 1.0
        kb = tb * tb * tb
        if same:
            rows = np.arange(k.shape[0])
            k[rows, at + rows] = 0
            kb[rows, at + rows] = 0
        total += k.sum(dtype=LD)
        bound += float(kb.sum())
    return total, bound


def three_sums(x, y):
    """-> (S [3] longdouble, B [3] float64): Sxx, Syy, Sxy."""
    parts = [sums(x, x, True), sums(y, y, True), sums(x, y)]
    return np.array([p[0] for p in parts], dtype=LD), np.array([p[1] for p in parts], dtype=np.float64)


def estimate(s, n, m):
    """KID from sums [..., 3] of sets of n and m rows, in the dtype of the sums."""
    s = np.asarray(s)
    return s[..., 0] / (n * (n - 1)) + s[..., 1] / (m * (m - 1)) - 2 * s[..., 2] / (n * m)


def estimate_bound(sum_bounds, s, n, m):
    """What bounds on the three sums imply for the estimate, plus the host's float64 roundings: one division and at most two additions behind
    every term, 3 u of the terms' magnitudes."""
    s = np.abs(np.asarray(s, dtype=np.float64))
    b = np.asarray(sum_bounds, dtype=np.float64)
    terms = s[..., 0] / (n * (n - 1)) + s[..., 1] / (m * (m - 1)) + 2 * s[..., 2] / (n * m)
    return b[..., 0] / (n * (n - 1)) + b[..., 1] / (m * (m - 1)) + 2 * b[..., 2] / (n * m) + 3 * U * terms


def draw_subsets(n, m, subsets, subset_size, seed):
    size = min(subset_size, n, m)
    rng = np.random.default_rng(seed)
    xi, yi = [], []
    for _ in range(subsets):
        xi.append(rng.choice(n, size, replace=False))
        yi.append(rng.choice(m, size, replace=False))
    return np.array(xi, dtype=np.int64).reshape(subsets, size), np.array(yi, dtype=np.int64).reshape(subsets, size)


def sum_bound(d, chain, bound_term):
    return U * (3 * d + 8 + chain) * np.asarray(bound_term, dtype=np.float64)


def figures(real, fake, subsets=100, subset_size=1000, seed=0):
    """-> dict(kid, subset_mean, subset_std, subset_kids, size: float64; sums [3], subset_sums [subsets, 3]: longdouble; sum_terms [3],
    subset_sum_terms [subsets, 3]: the bound terms)."""
    real, fake = np.asarray(real), np.asarray(fake)
    n, m = real.shape[0], fake.shape[0]
    full, full_terms = three_sums(real, fake)
    xi, yi = draw_subsets(n, m, subsets, subset_size, seed)
    size = xi.shape[1]
    parts = [three_sums(real[xi[s]], fake[yi[s]]) for s in range(subsets)]
    sub = np.array([p[0] for p in parts], dtype=LD).reshape(subsets, 3)
    sub_terms = np.array([p[1] for p in parts], dtype=np.float64).reshape(subsets, 3)
    kids = estimate(sub, size, size).astype(np.float64)
    return dict(kid=float(estimate(full, n, m)), subset_mean=float(kids.mean()) if subsets else float("nan"),
                subset_std=float(kids.std()) if subsets else float("nan"), subset_kids=kids, size=size, sums=full, subset_sums=sub, sum_terms=full_terms,
                subset_sum_terms=sub_terms)
