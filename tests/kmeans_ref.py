"""A numpy restatement of every rule of gansynth_amd/kmeans.py and of the three k-means entries (include/gansynth_hip.h), in float64 -- and,
with dtype=np.float32, the single-precision form of the same rules that says how far rounding alone moves a result.  Nothing here imports the
package: the tests hold the package against this file.

  sqdist        sum over the columns, ascending, of (x - c)^2 in `dtype` (the direct form; never the expansion)
  assign        argmin of it, np.argmin's tie rule (the lowest index)
  update        counts and the means of the non-empty clusters, the others untouched
  pick_next     the first row whose running float64 sum of dist exceeds u * total, clamped to n - 1
  relocate      empty clusters in index order <- the rows of largest dist, lowest index on ties
  lloyd/kmeans  assign; stop when nothing moved and nothing was relocated; update; relocate; a last assign after max_iter updates;
                the best of n_init runs by inertia, lowest run on ties; PCG64(seed + run), one random() per centre
  ndb           real counts from the labels, fake counts from one assign, the reference's pooled two-proportion z-test, and the JSD
"""
import functools

import numpy as np
import scipy.stats

U = 2.0 ** -24                     # fp32 unit round-off
MAX_K, TILE, MAX_SLICES = 256, 256, 512


def dist_bound(d):
    """Relative bound of a fp32 sum of d non-negative terms in any order, plus the rounding of each difference and square."""
    return (d + 8) * U


def sqdist(x, c, dtype=np.float64):
    """[n, k]: sum_j (x[i, j] - c[kk, j])^2, the columns in ascending order, every operation in `dtype`."""
    x, c = np.asarray(x, dtype=dtype), np.asarray(c, dtype=dtype)
    acc = np.zeros((x.shape[0], c.shape[0]), dtype=dtype)
    for j in range(x.shape[1]):
        t = x[:, j:j + 1] - c[None, :, j]
        acc += t * t
    return acc


def assign(x, c, dtype=np.float64):
    """-> (labels int32, dist: the minimum of sqdist, the matrix itself)."""
    full = sqdist(x, c, dtype)
    labels = np.argmin(full, axis=1).astype(np.int32)
    return labels, full[np.arange(len(labels)), labels], full


def ambiguous(full, d):
    """Rows whose best and second-best float64 distances lie within dist_bound(d) of each other: either label is right."""
    if full.shape[1] < 2:
        return np.zeros(full.shape[0], dtype=bool)
    two = np.partition(full, 1, axis=1)[:, :2]
    return two[:, 1] - two[:, 0] <= dist_bound(d) * (two[:, 1] + two[:, 0])


def update(x, labels, centres, dtype=np.float64):
    """-> (counts int64, new centres): the mean of every non-empty cluster, an empty one keeps its row of `centres`."""
    x = np.asarray(x, dtype=dtype)
    out = np.array(centres, dtype=dtype)
    counts = np.bincount(labels, minlength=len(out)).astype(np.int64)
    for kk in np.flatnonzero(counts):
        rows = x[labels == kk]
        out[kk] = (np.add.reduce(rows, axis=0, dtype=dtype) / dtype(len(rows))).astype(dtype)
    return counts, out


def pick_next(dist, u):
    values = [float(v) for v in np.asarray(dist, dtype=np.float64)]
    total = 0.0
    for v in values:                      # index order, float64
        total += v
    running, target = 0.0, u * total
    for i, v in enumerate(values):
        running += v
        if running > target:
            return i
    return len(values) - 1


def relocate(counts, dist):
    dist = np.asarray(dist, dtype=np.float64)
    taken, out = set(), []
    for cluster in range(len(counts)):
        if counts[cluster] != 0:
            continue
        best = None
        for i in range(len(dist)):
            if i not in taken and (best is None or dist[i] > dist[best]):   # strict: the lowest index on ties
                best = i
        taken.add(best)
        out.append((cluster, best))
    return out


def seed_rows(x, k, stream_seed, dtype=np.float64):
    rng = np.random.Generator(np.random.PCG64(stream_seed))
    n = len(x)
    rows = [min(int(np.floor(rng.random() * n)), n - 1)]
    dist = None
    for _ in range(1, k):
        new = sqdist(x, np.asarray(x)[rows[-1]][None], dtype)[:, 0]
        dist = new if dist is None else np.minimum(dist, new)
        rows.append(pick_next(dist.astype(np.float32) if dtype == np.float32 else dist, rng.random()))
    return rows


def lloyd(x, centres, max_iter, dtype=np.float64, log=None):
    """-> (labels, inertia, iterations, centres).  `log` (a list) receives every relocation [(cluster, row)]."""
    centres = np.array(centres, dtype=dtype)
    labels = np.full(len(x), -1, dtype=np.int32)
    relocated, iterations = False, 0
    for _ in range(max_iter):
        new, dist, _ = assign(x, centres, dtype)
        changed = int(np.count_nonzero(new != labels))
        labels = new
        if changed == 0 and not relocated:
            return labels, float(np.sum(dist, dtype=np.float64)), iterations, centres
        counts, centres = update(x, labels, centres, dtype)
        moves = relocate(counts, dist)
        for cluster, row in moves:
            centres[cluster] = np.asarray(x, dtype=dtype)[row]
        if moves and log is not None:
            log.append(moves)
        relocated = bool(moves)
        iterations += 1
    labels, dist, _ = assign(x, centres, dtype)
    return labels, float(np.sum(dist, dtype=np.float64)), iterations, centres


def kmeans(x, k, seed=0, n_init=10, max_iter=300, init=None, dtype=np.float64):
    """-> dict(centres, labels, counts, inertia, iterations, run, seed_rows, inertias: every run's)."""
    best, inertias = None, []
    for run in range(1 if init is not None else n_init):
        rows = None if init is not None else seed_rows(x, k, seed + run, dtype)
        start = np.asarray(init) if init is not None else np.asarray(x)[rows]
        labels, inertia, iterations, centres = lloyd(x, start, max_iter, dtype)
        inertias.append(inertia)
        if best is None or inertia < best["inertia"]:
            best = dict(centres=centres, labels=labels, counts=np.bincount(labels, minlength=k), inertia=inertia, iterations=iterations, run=run,
                        seed_rows=rows)
    best["inertias"] = inertias
    return best


def kl(p, q):
    return float(sum(a * np.log(a / b) for a, b in zip(p, q) if a > 0.0))


def jsd(p, q):
    p, q = np.asarray(p, dtype=np.float64), np.asarray(q, dtype=np.float64)
    m = 0.5 * (p + q)
    return 0.5 * kl(p, m) + 0.5 * kl(q, m)


def different_bins(real_counts, fake_counts, significance_level=0.05):
    """The reference's test (metrics.py:33-38): z = (pooled - q) / se with the pooled standard error."""
    m, n = int(np.sum(real_counts)), int(np.sum(fake_counts))
    p, q = np.asarray(real_counts) / m, np.asarray(fake_counts) / n
    pooled = (p * m + q * n) / (m + n)
    with np.errstate(divide="ignore", invalid="ignore"):
        z = (pooled - q) / np.sqrt(pooled * (1.0 - pooled) * (1.0 / m + 1.0 / n))
    return int(np.count_nonzero(scipy.stats.norm.cdf(-np.abs(z)) * 2.0 < significance_level))


def ndb(real, fake, num_bins=50, significance_level=0.05, seed=0, n_init=10, dtype=np.float64):
    """-> (count, dict(real_counts, fake_counts, inertia, jsd))."""
    fit = kmeans(real, num_bins, seed=seed, n_init=n_init, dtype=dtype)
    fake_counts = np.bincount(assign(fake, fit["centres"], dtype)[0], minlength=num_bins)
    details = dict(real_counts=fit["counts"], fake_counts=fake_counts, inertia=fit["inertia"],
                   jsd=jsd(fit["counts"] / fit["counts"].sum(), fake_counts / fake_counts.sum()))
    return different_bins(fit["counts"], fake_counts, significance_level), details


def workspace_bytes(n, d, k):
    """gs_kmeans_workspace_bytes as include/gansynth_hip.h states it."""
    s0 = max(1, min(MAX_SLICES, 2048 // -(-d // 64), -(-n // 64)))
    slices = -(-n // -(-n // s0))
    return -(-max(12 * -(-n // TILE), 4 * slices * k * (d + 1)) // 16) * 16


# ---------------------------------------------------------------------------------------------------------------- inputs
def mixture(n, d, k, separation, seed, offset=4.0):
    """n fp32 rows of a k-component unit-variance Gaussian mixture whose means are N(offset, separation^2) per column: features with a common
    offset, as the classifier's post-ReLU means have.  -> (x [n, d] fp32, the component of every row)."""
    rng = np.random.default_rng(seed)
    means = offset + separation * rng.standard_normal((k, d))
    comp = rng.integers(0, k, n)
    return (means[comp] + rng.standard_normal((n, d))).astype(np.float32), comp


# (n, d, k, separation): the four inputs of the algorithm tests
CASES = {"2049x65x7": (2049, 65, 7, 1.0), "1500x512x50": (1500, 512, 50, 0.5), "4096x512x50": (4096, 512, 50, 0.75), "3000x16x10": (3000, 16, 10, 1.0)}


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (x, init: k rows of x drawn without replacement) of a named case; seeded by the name's position."""
    n, d, k, separation = CASES[name]
    seed = 100 + list(CASES).index(name)
    x, _ = mixture(n, d, k, separation, seed)
    init = x[np.random.default_rng(seed + 50).choice(n, k, replace=False)].copy()
    x.setflags(write=False)
    init.setflags(write=False)
    return x, init


@functools.lru_cache(maxsize=None)
def case_lloyd(name, single=False):
    """lloyd from the case's init, in float64 or (single) float32: computed once, shared, not to be written to."""
    x, init = case(name)
    return lloyd(x, init, 300, np.float32 if single else np.float64)
