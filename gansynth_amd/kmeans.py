"""k-means on the device, for the NDB metric (metrics.num_different_bins_device; DESIGN.md "NDB on the device").

The reference's metrics.py leaves the clustering to scikit-learn, whose random stream cannot be reproduced; the rules below are this project's
own, and tests/kmeans_ref.py restates every one of them in float64 numpy.

  Distances   squared Euclidean, sum over the columns of (x - c)^2 in fp32 (gs_kmeans_assign); ties to the lowest centre index.
  Seeding     plain k-means++, one trial per centre, once per run r = 0 .. n_init - 1.  The uniforms come from
              np.random.Generator(np.random.PCG64(seed + r)), one random() per centre.  The first centre is row floor(u n).  Each later one is
              pick_next(dist, u): the first row whose running sum of dist exceeds u * total, clamped to n - 1 -- the running sum taken on the
              host in float64 over the fp32 values of gs_kmeans_mindist, in index order.  `init` (a [k, d] array) replaces the seeding and forces
              one run.
  Iteration   assign; stop when no label moved and nothing was relocated in the iteration before; otherwise update (the mean of every non-empty
              cluster, gs_kmeans_update) and relocate.  `iterations` counts the updates.  After max_iter of them one last assign makes the labels
              agree with the returned centres.
  Relocation  relocate_empty(counts, dist): the empty clusters, in index order, each take the row with the largest current dist (the distances
              of the assign before the update) not yet taken, the lowest index on ties; that row becomes the centre.  A rare path.
  Best run    the lowest inertia, the lowest run index on ties.  The inertia is the sum over the rows of the distance to the centre taken, every
              term and every sum in double on the device (gs_kmeans_inertia, one read of x at the end of a run): two runs that reach the same
              partition reach the same bits, and the choice between runs carries no fp32 rounding.
"""
import collections

import numpy as np
import torch

from . import kernels

KMeansResult = collections.namedtuple("KMeansResult", "centres labels counts inertia iterations run seed_rows")
KMeansResult.__doc__ = """centres [k, d] fp32 and labels [n] int32 on the device; counts [k] int64 (numpy): the rows of every label; inertia (float);
iterations: the updates of the best run; run: its index; seed_rows: the rows its k-means++ picked (None with `init`)."""


def pick_next(dist, u):
    """The k-means++ draw: the first row whose running sum of `dist` (float64, index order) exceeds u * total, clamped to the last row."""
    running = np.cumsum(np.asarray(dist, dtype=np.float64))
    return int(min(np.searchsorted(running, u * running[-1], side="right"), len(running) - 1))


def relocate_empty(counts, dist):
    """[(cluster, row)] for the empty clusters in index order: each takes the row with the largest `dist` not yet taken, lowest index on ties."""
    empty = np.flatnonzero(np.asarray(counts) == 0)
    if len(empty) == 0:
        return []
    order = np.argsort(-np.asarray(dist, dtype=np.float64), kind="stable")
    if len(empty) > len(order):
        raise ValueError(f"relocate_empty: {len(empty)} empty clusters but only {len(order)} rows")
    return [(int(c), int(r)) for c, r in zip(empty, order[:len(empty)])]


def to_device(x, name="x"):
    """x (numpy or torch, [n, d]) as fp32 on the device: the one copy."""
    if not isinstance(x, torch.Tensor):
        x = np.ascontiguousarray(x)
        x = torch.from_numpy(x if x.flags.writeable else x.copy())   # (torch refuses to wrap a read-only array quietly)
    t = x
    if t.dim() != 2 or t.numel() == 0:
        raise ValueError(f"kmeans: {name} must be a non-empty [rows, columns] matrix (got {tuple(t.shape)})")
    if not t.is_cuda:
        t = t.to("cuda")
    return t.to(torch.float32)


def seed_rows(x, k, rng):
    """k-means++ on the device rows x with the uniforms of `rng`: -> the k rows picked."""
    n = x.shape[0]
    rows = [min(int(np.floor(rng.random() * n)), n - 1)]
    dist = None
    for _ in range(1, k):
        dist = kernels.kmeans_mindist(x, x[rows[-1]].contiguous(), dist)
        rows.append(pick_next(dist.cpu().numpy(), rng.random()))
    return rows


def lloyd(x, centres, max_iter):
    """Lloyd's iteration from `centres` ([k, d] fp32 on the device, overwritten): -> (labels, inertia, iterations)."""
    n = x.shape[0]
    labels = torch.full((n,), -1, dtype=torch.int32, device=x.device)
    relocated, iterations, converged = False, 0, False
    for _ in range(max_iter):
        _, dist, changed, _ = kernels.kmeans_assign(x, centres, labels=labels)
        if int(changed.item()) == 0 and not relocated:
            converged = True
            break
        counts = kernels.kmeans_update(x, labels, centres).cpu().numpy()
        moves = relocate_empty(counts, dist.cpu().numpy()) if (counts == 0).any() else []
        for cluster, row in moves:
            centres[cluster].copy_(x[row])
        relocated = bool(moves)
        iterations += 1
    if not converged:   # max_iter updates: one last assign moves the labels onto the returned centres
        kernels.kmeans_assign(x, centres, labels=labels, want_dist=False)
    return labels, float(kernels.kmeans_inertia(x, centres, labels).item()), iterations


def kmeans(x, k, seed=0, n_init=10, max_iter=300, init=None):
    """The module's rules on x ([n, d], numpy or torch; moved to the device as fp32 once): -> KMeansResult."""
    x = to_device(x)
    n, d = x.shape
    if not isinstance(k, (int, np.integer)) or not 1 <= k <= min(n, kernels._lib.KMEANS_MAX_K):
        raise ValueError(f"kmeans: k must be an integer in [1, min(rows, {kernels._lib.KMEANS_MAX_K})] (got {k!r} for {n} rows)")
    if max_iter < 0 or (init is None and n_init < 1):
        raise ValueError(f"kmeans: max_iter must be >= 0 and n_init >= 1 (got {max_iter}, {n_init})")
    if init is not None:
        start = to_device(init, "init").to(x.device)
        if tuple(start.shape) != (k, d):
            raise ValueError(f"kmeans: init must be [{k}, {d}] (got {tuple(start.shape)})")
    best = None
    for run in range(1 if init is not None else n_init):
        if init is not None:
            rows, centres = None, start.clone().contiguous()
        else:
            rows = seed_rows(x, k, np.random.Generator(np.random.PCG64(seed + run)))
            centres = x[torch.as_tensor(rows, device=x.device)].contiguous()
        labels, inertia, iterations = lloyd(x, centres, max_iter)
        if best is None or inertia < best.inertia:
            best = KMeansResult(centres, labels, None, inertia, iterations, run, rows)
    counts = torch.bincount(best.labels.long(), minlength=k).cpu().numpy()
    return best._replace(counts=counts)
