"""GPU: gs_knn_kth / gs_knn_within element-wise against the float64 restatement (tests/knn_ref.py), then manifold / metrics.precision_recall_device,
GANSynth.evaluate(prd=True) and the driver's --prd.  Every figure is printed before it is asserted.

The kernel tests call the C entries themselves: the inputs sit inside NaN-filled buffers with row slack (lda = d + 3), once 16-byte aligned and
once one float off, every output inside a sentinel-filled buffer, and nothing outside the outputs may change.

Bounds (u = 2^-24): a distance is a fp32 sum of d non-negative terms, each a rounded square of a rounded difference: within (d + 8) u, relative,
of its float64 value (kmeans_ref.dist_bound).  An order statistic is monotone in every distance, so the j-th smallest fp32 distance lies within
that bound of the j-th smallest float64 one: no exception rule.  A count must lie in [sure, sure + ambiguous], `ambiguous` the pairs whose float64
distance is within the bound of the radius (knn_ref.ambiguous_pairs), `sure` the others inside; ambiguous pairs may be at most 0.1 % of a case's
pairs.  The inputs are seeded rows around 8 shared centres with a common offset of 4; on every one of them the fp32 numpy restatement disagrees
with float64 on no pair, and at most 4 pairs of a case (of 159 177, at d = 513) are ambiguous (checked on the CPU; the tests print the count and
hold the cap)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import kmeans_ref as KR
from tests import knn_ref as NR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = KR.TILE
PAD = 64                                   # floats of sentinel on either side of every buffer
I_SENT, F_SENT = -7777, -12345.5
# (d, n, m, k): every d of {1, 3, 65, 512, 513}; n and m below, at and past a tile and past two; k of {1, 3, 5, 8}; one slice and several
SHAPES = [(1, 2, 2, 1), (3, T - 1, T + 1, 3), (65, T, 300, 3), (512, T + 1, 64, 8), (513, 2 * T + 35, 291, 5), (3, 1024, 1024, 3), (65, 9, 9, 8),
          (512, 5, 2 * T + 35, 1)]
IDS = [f"d{d}-n{n}-m{m}-k{k}" for d, n, m, k in SHAPES]


def _lib():
    from gansynth_amd import _lib as L
    return L, L.load()


@functools.lru_cache(maxsize=None)
def _inputs(d, n, m):
    """-> (a [n, d], b [m, d]) fp32, read-only: seeded by the shape, rows around 8 shared centres."""
    rng = np.random.default_rng(100000 * d + 100 * n + m)
    a, centres = NR.clustered(n, d, rng)
    b, _ = NR.clustered(m, d, rng, centres)
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


@functools.lru_cache(maxsize=None)
def _kth64(d, n, m, k, self_):
    a, b = _inputs(d, n, m)
    out = NR.kth(a, a, k, True) if self_ else NR.kth(a, b, k, False)
    out.setflags(write=False)
    return out


def _place(a, aligned, slack=3):
    """a [n, d] inside a NaN-filled device buffer, rows d + slack apart, the first on 16 bytes or one float off: -> (buffer, view, ld)."""
    n, d = a.shape
    ld = d + slack
    off = PAD + (0 if aligned else 1)
    buf = torch.full((off + n * ld + PAD,), float("nan"), device="cuda")
    view = buf[off:off + n * ld].view(n, ld)[:, :d]
    view.copy_(torch.from_numpy(np.array(a)))                 # (a copy: the shared inputs are read-only)
    assert (view.data_ptr() % 16 == 0) == aligned
    return buf, view, ld


def _out(count, sentinel, dtype, aligned=True):
    """`count` elements inside a sentinel-filled buffer: -> (buffer, view)."""
    off = PAD + (0 if aligned else 1)
    buf = torch.full((off + count + PAD,), sentinel, dtype=dtype, device="cuda")
    return buf, buf[off:off + count]


def _intact(buf, view, sentinel):
    """Nothing around `view` inside `buf` was written."""
    host = buf.cpu().numpy()
    off = (view.data_ptr() - buf.data_ptr()) // buf.element_size()
    return bool((host[:off] == sentinel).all() and (host[off + view.numel():] == sentinel).all())


def _kth(av, lda, bv, ldb, k, exclude, out):
    from gansynth_amd import kernels
    L, lib = _lib()
    (n, d), m = av.shape, bv.shape[0]
    ws = kernels._ws(lib.gs_knn_workspace_bytes(n, m, d, k), torch.device("cuda"))
    L.check(lib.gs_knn_kth(av.data_ptr(), lda, n, bv.data_ptr(), ldb, m, d, k, 1 if exclude else 0, out.data_ptr(), ws.data_ptr(), ws.numel(),
                           kernels._stream()), "gs_knn_kth")
    torch.cuda.synchronize()


def _within(qv, ldq, rv, ldr, radius2, count):
    from gansynth_amd import kernels
    L, lib = _lib()
    (n, d), m = qv.shape, rv.shape[0]
    ws = kernels._ws(lib.gs_knn_workspace_bytes(n, m, d, 1), torch.device("cuda"))
    L.check(lib.gs_knn_within(qv.data_ptr(), ldq, n, rv.data_ptr(), ldr, m, d, radius2.data_ptr(), count.data_ptr(), ws.data_ptr(), ws.numel(),
                              kernels._stream()), "gs_knn_within")
    torch.cuda.synchronize()


def test_the_shapes_cover_one_slice_and_several():
    L, lib = _lib()
    slices = [(lib.gs_knn_slices(n, m, d), lib.gs_knn_slices(n, n, d)) for d, n, m, _ in SHAPES]
    print("slices (cross, self) per shape:", slices)
    flat = [s for pair in slices for s in pair]
    assert min(flat) == 1 and max(flat) > 2 and all(s == NR.slices(n, m) for (s, _), (_, n, m, _) in zip(slices, SHAPES))


# ----------------------------------------------------------------------------------------------------------------- kth
def _check_kth(got, want, d, what):
    finite = np.isfinite(want)
    err = np.abs(got[finite] - want[finite]) / np.maximum(want[finite], 1e-300)
    print(f"{what}: worst error {err.max() if err.size else 0.0:.3g} relative to the float64 order statistic (bound {KR.dist_bound(d):.3g}); "
          f"{int((~finite).sum())} +inf places")
    assert np.array_equal(np.isposinf(got), ~finite)                                     # +inf exactly where the candidates run out
    assert (np.abs(got[finite] - want[finite]) <= KR.dist_bound(d) * want[finite]).all()
    with np.errstate(invalid="ignore"):
        assert (np.diff(got, axis=1) >= 0)[np.isfinite(got[:, 1:])].all()                  # ascending


@pytest.mark.parametrize("d,n,m,k", SHAPES, ids=IDS)
def test_kth(d, n, m, k):
    a, b = _inputs(d, n, m)
    results = {}
    for aligned in (True, False):
        abuf, av, lda = _place(a, aligned)
        bbuf, bv, ldb = _place(b, aligned)
        for self_ in (True, False):
            obuf, out = _out(n * k, F_SENT, torch.float32, aligned)
            _kth(av, lda, av if self_ else bv, lda if self_ else ldb, k, self_, out)
            got = out.view(n, k).cpu().numpy().astype(np.float64)
            if aligned:
                _check_kth(got, _kth64(d, n, m, k, self_), d, f"d {d} n {n} m {m} k {k} {'self' if self_ else 'cross'}")
            assert _intact(obuf, out, F_SENT)
            again_buf, again = _out(n * k, F_SENT, torch.float32, aligned)
            _kth(av, lda, av if self_ else bv, lda if self_ else ldb, k, self_, again)
            assert torch.equal(again, out)                                                 # two calls: the same bits
            results[(aligned, self_)] = out.clone()
        assert np.isnan(abuf.cpu().numpy()).sum() == abuf.numel() - n * d and np.isnan(bbuf.cpu().numpy()).sum() == bbuf.numel() - m * d
    for self_ in (True, False):
        assert torch.equal(results[(True, self_)], results[(False, self_)])               # the two placements: the same bits
    if n - 1 == k:                                                                         # n = 2, k = 1 and (65, 9, 9, 8): exactly k other rows
        assert np.isfinite(results[(True, True)].cpu().numpy()).all()


def test_kth_fills_with_inf_where_the_candidates_run_out():
    """Five rows of the (65, 9, 9) input against themselves at k = 8: four candidates a row; against two rows of b at k = 3: two."""
    d, k = 65, 8
    a, b = (x[:5] for x in _inputs(65, 9, 9))
    _, av, lda = _place(a, False)
    _, bv, ldb = _place(b[:2], True)
    obuf, out = _out(5 * k, F_SENT, torch.float32)
    _kth(av, lda, av, lda, k, True, out)
    own = out.view(5, k).cpu().numpy().astype(np.float64)
    _check_kth(own, NR.kth(a, a, k, True), d, "5 rows, self, k 8")
    assert np.isfinite(own[:, :4]).all() and np.isposinf(own[:, 4:]).all() and _intact(obuf, out, F_SENT)
    obuf, out = _out(5 * 3, F_SENT, torch.float32)
    _kth(av, lda, bv, ldb, 3, False, out)
    cross = out.view(5, 3).cpu().numpy().astype(np.float64)
    _check_kth(cross, NR.kth(a, b[:2], 3, False), d, "5 rows against 2, k 3")
    assert np.isfinite(cross[:, :2]).all() and np.isposinf(cross[:, 2]).all() and _intact(obuf, out, F_SENT)


def test_kth_duplicate_rows_give_an_exact_zero():
    """Row 3 repeated at row T + 5 (another tile) and in b: only the index excludes, so both copies see a neighbour at distance 0."""
    d, n, m, k = 65, T + 9, 300, 3
    a, b = (np.array(x) for x in _inputs(d, T + 1, 300))
    a = np.concatenate([a, a[:8] + np.float32(0.25)])
    a[T + 5] = a[3]
    b[17] = a[3]
    _, av, lda = _place(a, False)
    _, bv, ldb = _place(b, True)
    obuf, out = _out(n * k, F_SENT, torch.float32)
    _kth(av, lda, av, lda, k, True, out)
    own = out.view(n, k).cpu().numpy()
    _kth(av, lda, bv, ldb, k, False, out)
    cross = out.view(n, k).cpu().numpy()
    print(f"self: rows 3 and {T + 5} start with {own[3, 0]!r}, {own[T + 5, 0]!r}; zeros elsewhere {int((own[:, 0] == 0).sum()) - 2}; cross: {cross[3, 0]!r}, {cross[T + 5, 0]!r}")
    assert own[3, 0] == 0.0 and own[T + 5, 0] == 0.0 and (own[:, 0] == 0).sum() == 2 and (own[:, 1] > 0).all()
    assert cross[3, 0] == 0.0 and cross[T + 5, 0] == 0.0 and (cross[:, 0] == 0).sum() == 2
    _check_kth(own.astype(np.float64), NR.kth(a, a, k, True), d, "duplicates, self")


# ----------------------------------------------------------------------------------------------------------------- within
def _bracket(got, q, ref, radius2, d, what):
    """sure <= count <= sure + ambiguous, from float64: -> the number of ambiguous pairs (at most 0.1 % of the pairs)."""
    amb = NR.ambiguous_pairs(q, ref, radius2, d)
    with np.errstate(invalid="ignore"):
        inside = KR.sqdist(q, ref) <= np.asarray(radius2, dtype=np.float64)[None, :]
    sure = (inside & ~amb).sum(axis=1)
    maybe = amb.sum(axis=1)
    single = NR.within(q, ref, radius2, np.float32)
    print(f"{what}: {int(amb.sum())} ambiguous pairs of {amb.size} (cap {0.001 * amb.size:.3f}); counts differ from float64 on {int((got != inside.sum(axis=1)).sum())} "
          f"rows (fp32 restatement: {int((single != inside.sum(axis=1)).sum())}); sum {int(got.sum())}")
    assert amb.sum() <= 0.001 * amb.size
    assert (sure <= got).all() and (got <= sure + maybe).all()
    return int(amb.sum())


@pytest.mark.parametrize("d,n,m,k", SHAPES, ids=IDS)
def test_within(d, n, m, k):
    q, ref = _inputs(d, n, m)
    results = {}
    for aligned in (True, False):
        qbuf, qv, ldq = _place(q, aligned)
        rbuf, rv, ldr = _place(ref, aligned)
        kk = min(k, m - 1)                                                                 # (a radius needs kk other rows)
        rad_buf, radii = _out(m * kk, F_SENT, torch.float32)
        _kth(rv, ldr, rv, ldr, kk, True, radii)                                            # the fp32 radii of ref, from the device
        radius2 = radii.view(m, kk)[:, kk - 1].contiguous()
        cbuf, count = _out(n, I_SENT, torch.int32, aligned)
        _within(qv, ldq, rv, ldr, radius2, count)
        got = count.cpu().numpy()
        assert count.dtype == torch.int32 and _intact(cbuf, count, I_SENT)
        if aligned:
            _bracket(got, q, ref, radius2.cpu().numpy(), d, f"d {d} n {n} m {m} k {kk}")
        again_buf, again = _out(n, I_SENT, torch.int32, aligned)
        _within(qv, ldq, rv, ldr, radius2, again)
        assert torch.equal(again, count)
        results[aligned] = count.clone()
        # NaN admits nothing, +inf every row, the others as before
        special = radius2.clone()
        special[0] = float("nan")
        special[m - 1] = float("inf")
        _within(qv, ldq, rv, ldr, special, again)
        zeroed = radius2.clone()
        zeroed[0] = -1.0
        zeroed[m - 1] = -1.0
        base_buf, base = _out(n, I_SENT, torch.int32, aligned)
        _within(qv, ldq, rv, ldr, zeroed, base)                                            # (a negative radius admits nothing either)
        assert torch.equal(again, base + 1) and _intact(again_buf, again, I_SENT)
        assert np.isnan(qbuf.cpu().numpy()).sum() == qbuf.numel() - n * d
    assert torch.equal(results[True], results[False])


# ----------------------------------------------------------------------------------------------------------------- one distance, one set of bits
def test_within_admits_exactly_the_pairs_kth_returned():
    """(65, 9, 9): the [9, 8] matrix of gs_knn_kth holds every distance of every row to the 8 others.  d(i, j) and d(j, i) are the same bits, so
    count[i] = 1 (the pair with itself: 0 <= R) + #{j != i : d(i, j) <= R(j)} can be derived on the host from that matrix and the radii alone --
    as multisets: row j's list is the distances d(j, .) = d(., j), and how many of ALL rows' lists' entries lie within R(j) says how many rows lie
    in ball j."""
    d, n, k = 65, 9, 3
    a, _ = _inputs(d, n, n)
    _, av, lda = _place(a, True)
    _, full = _out(n * 8, F_SENT, torch.float32)
    _kth(av, lda, av, lda, 8, True, full)
    lists = full.view(n, 8).cpu().numpy()                      # row j: its distances to the 8 others, ascending
    radius2 = np.ascontiguousarray(lists[:, k - 1])
    _, count = _out(n, I_SENT, torch.int32)
    _within(av, lda, av, lda, torch.from_numpy(radius2).cuda(), count)
    got = count.cpu().numpy()
    # ball j holds row j and the k rows nearest to it (more on a tie): the entries of ITS list within its radius.  Summed over j that is the sum
    # of the counts; and row i lies in ball j iff d(j, i) <= R(j), where d(j, i) is an entry of list j AND, the same bits, of list i.
    in_ball = 1 + (lists <= radius2[:, None]).sum(axis=1)      # rows in ball j
    # per row: match every entry of list i to the row j it belongs to through the float64 order (no ties at these inputs), then compare in fp32
    order = np.argsort(np.where(np.eye(n, dtype=bool), np.inf, KR.sqdist(a, a)), axis=1, kind="stable")[:, :8]
    want = np.ones(n, dtype=np.int64)
    for i in range(n):
        for place, j in enumerate(order[i]):
            want[i] += lists[i, place] <= radius2[j]
    print(f"counts {got.tolist()}, derived on the host {want.tolist()}; rows per ball {in_ball.tolist()}")
    assert np.array_equal(got, want) and got.sum() == in_ball.sum()
    for i in range(n):                                         # the symmetry itself: d(i, j) in list i is, bit for bit, an entry of list j
        for place, j in enumerate(order[i]):
            assert lists[i, place] == lists[j, list(order[j]).index(i)]


@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "one float off"])
@pytest.mark.parametrize("d", [1, 33, 64])
def test_assign_and_knn_share_one_distance(d, aligned):
    """gs_kmeans_assign, gs_knn_kth and gs_knn_within add d(i, j) through the one chain of csrc/pairs_tile.h (assign in its scalar form, k-NN in
    its packed form), so on inputs without NaN every figure below is an equality of bits: no tolerance.  n = T + 1 rows (one past a tile);
    d below a chunk of 32 columns, one past it and two whole chunks; k = 1, 16, 32, 50, 65, 256 centres: assign's KG = 4, 4, 8, 13, 13 in two
    rounds and 16 in four, and one to four k-NN rounds of 64 (five, the last with one row, where x is the other side).
      * assign's dist is knn_kth(x, c, 1), the minimum over the same centres.
      * The counts of knn_within(x, c, R), R[j] = knn_kth(c, x, 1)[j] centre j's own radius (the distance to its nearest row, x now the
        broadcast side), are recomputed on the host.  The minima alone do not hold the k - 1 other distances of a row, so the host takes all of
        d(., j) from the device as assign's dist against centre j alone, which is that chain again: the row minimum of that matrix must be
        dist, its first arg-minimum the label, its column minimum R."""
    from gansynth_amd import kernels
    n = T + 1
    rng = np.random.default_rng(5000 + d)
    x, centres = NR.clustered(n, d, rng)
    _, xv, _ = _place(x, aligned)
    for k in (1, 16, 32, 50, 65, 256):
        c = NR.clustered(k, d, rng, centres)[0]
        _, cflat = _out(k * d, F_SENT, torch.float32, aligned)                               # (assign takes contiguous centres: no row slack)
        cv = cflat.view(k, d)
        cv.copy_(torch.from_numpy(c))
        assert (cv.data_ptr() % 16 == 0) == aligned
        labels, dist, _, _ = kernels.kmeans_assign(xv, cv)
        nearest = kernels.knn_kth(xv, cv, 1)[:, 0]
        assert torch.equal(dist, nearest)
        full = torch.stack([kernels.kmeans_assign(xv, cv[j:j + 1])[1] for j in range(k)], dim=1).cpu().numpy()   # [n, k]
        radius2 = kernels.knn_kth(cv, xv, 1)[:, 0].contiguous()
        count = kernels.knn_within(xv, cv, radius2).cpu().numpy()
        want = (full <= radius2.cpu().numpy()[None, :]).sum(axis=1)
        print(f"d {d} k {k}: dist from {float(dist.min()):.6g} to {float(dist.max()):.6g}; rows inside a centre's radius {int((count > 0).sum())}, "
              f"pairs {int(count.sum())} (host {int(want.sum())})")
        assert np.array_equal(full.min(axis=1), dist.cpu().numpy()) and np.array_equal(full.argmin(axis=1), labels.cpu().numpy())
        assert np.array_equal(full.min(axis=0), radius2.cpu().numpy())
        assert np.array_equal(count, want) and count.sum() >= k                              # (every centre's nearest row lies AT its radius)


@functools.lru_cache(maxsize=None)
def _clean_set(d, n, k):
    """The first seed whose n rows have, in float64, no pair other than the n k defining ones within the bound of a radius."""
    for seed in range(50):
        a, _ = NR.clustered(n, d, np.random.default_rng(7000 + seed))
        radius2 = NR.kth(a, a, k, True)[:, k - 1]
        full = KR.sqdist(a, a)
        # (here BOTH sides are rounded on the device, the distance and the radius: the margin is the sum of the two bounds, and a half more)
        amb = np.abs(full - radius2[None, :]) <= 2.5 * KR.dist_bound(d) * np.maximum(full, radius2[None, :])
        defining = (full == radius2[None, :]) & ~np.eye(n, dtype=bool)
        inside = (full <= radius2[None, :]).sum()
        if defining.sum() == n and not (amb & ~defining).any() and inside == n * (k + 1):
            return seed, a
    raise AssertionError("no seed gives a set without ambiguous pairs")


def test_a_radius_admits_its_own_neighbours():
    """(65, T + 1), k = 3: every ball holds its row and its 3 nearest -- the defining pair at EXACTLY the radius, which only one set of bits for
    d(i, j) and d(j, i) admits -- and, at this seed, nothing else is near a radius: sum(count) = n (k + 1)."""
    d, n, k = 65, T + 1, 3
    seed, a = _clean_set(d, n, k)
    _, av, lda = _place(a, False)
    _, radii = _out(n * k, F_SENT, torch.float32)
    _kth(av, lda, av, lda, k, True, radii)
    radius2 = radii.view(n, k)[:, k - 1].contiguous()
    cbuf, count = _out(n, I_SENT, torch.int32)
    _within(av, lda, av, lda, radius2, count)
    got = count.cpu().numpy()
    print(f"seed {7000 + seed}: counts from {got.min()} to {got.max()}, sum {got.sum()} (n (k + 1) = {n * (k + 1)})")
    assert (got >= 1).all() and got.sum() == n * (k + 1) and _intact(cbuf, count, I_SENT)


# ----------------------------------------------------------------------------------------------------------------- manifold and metrics
def test_python_layer_matches_the_entries():
    from gansynth_amd import kernels
    d, n, m, k = 65, T, 300, 3
    a, b = _inputs(d, n, m)
    _, av, lda = _place(a, False)
    _, bv, ldb = _place(b, True)
    _, out = _out(n * k, F_SENT, torch.float32)
    _kth(av, lda, bv, ldb, k, False, out)
    assert torch.equal(kernels.knn_kth(av, bv, k), out.view(n, k))                          # views with row slack are taken as they stand
    _kth(av, lda, av, lda, k, True, out)
    own = kernels.knn_kth(av, av, k, exclude_diagonal=True)
    assert torch.equal(own, out.view(n, k)) and torch.equal(kernels.knn_kth(torch.from_numpy(np.array(a)).cuda(), av, k, exclude_diagonal=True), own)
    radius2 = own[:, k - 1].contiguous()
    _, count = _out(m, I_SENT, torch.int32)
    _within(bv, ldb, av, lda, radius2, count)
    got = kernels.knn_within(bv, av, radius2)
    assert got.dtype == torch.int32 and torch.equal(got, count)
    with pytest.raises(ValueError, match="x must be on the HIP device"):
        kernels.knn_kth(torch.from_numpy(np.array(a)), bv, k)
    with pytest.raises(ValueError, match="b is on cpu"):
        kernels.knn_kth(av, torch.from_numpy(np.array(b)), k)
    with pytest.raises(ValueError, match="radius2 is on cpu"):
        kernels.knn_within(bv, av, radius2.cpu())


def test_precision_recall_device_against_the_restatement():
    """600 x 64 against 500 x 64, the fake set shifted a little: the counts bracket as in test_within, and a figure, a quotient by the rows, moves by
    at most (ambiguous pairs or rows) / rows (coverage: a row is ambiguous when its float64 minimum and radius lie within the sum of their two
    roundings of each other)."""
    from gansynth_amd import metrics
    rng = np.random.default_rng(42)
    real, centres = NR.clustered(600, 64, rng)
    fake = NR.clustered(500, 64, rng, centres)[0] + np.float32(0.05)
    want = NR.figures(real, fake, 3)
    details = {}
    got = metrics.precision_recall_device(real, torch.from_numpy(fake), k=3, details=details)
    keys = ("precision", "recall", "density", "coverage")
    print("device     ", {key: got[key] for key in keys})
    print("restatement", {key: want[key] for key in keys})
    assert set(got) == set(keys) and all(isinstance(got[key], float) for key in keys)
    for name, ref in (("real_radii", want["real_radii"]), ("fake_radii", want["fake_radii"]), ("coverage_minima", want["coverage_minima"])):
        assert details[name].dtype == np.float32 and (np.abs(details[name].astype(np.float64) - ref) <= KR.dist_bound(64) * ref).all(), name
    amb_fake = _bracket(details["fake_counts"], fake, real, details["real_radii"], 64, "fake rows in real balls")
    amb_real = _bracket(details["real_counts"], real, fake, details["fake_radii"], 64, "real rows in fake balls")
    minima64 = want["coverage_minima"]
    amb_cover = int((np.abs(minima64 - want["real_radii"]) <= KR.dist_bound(64) * (minima64 + want["real_radii"])).sum())   # (both sides carry a rounding)
    print(f"ambiguous: {amb_fake} pairs for precision / density, {amb_real} for recall, {amb_cover} rows for coverage")
    # (the device's radii are fp32 roundings of the float64 ones; a pair whose float64 distance lies between the two is counted here, for the
    #  reader: such a pair is within the bound of the radius, so it is ambiguous in the sense above as well)
    moved_fake = int(((KR.sqdist(fake, real) <= want["real_radii"][None, :]) != (KR.sqdist(fake, real) <= details["real_radii"].astype(np.float64)[None, :])).sum())
    moved_real = int(((KR.sqdist(real, fake) <= want["fake_radii"][None, :]) != (KR.sqdist(real, fake) <= details["fake_radii"].astype(np.float64)[None, :])).sum())
    print(f"pairs that the rounding of the radii moves: {moved_fake}, {moved_real}")
    assert abs(got["precision"] - want["precision"]) <= amb_fake / 500
    assert abs(got["density"] - want["density"]) <= amb_fake / (3 * 500)
    assert abs(got["recall"] - want["recall"]) <= amb_real / 600
    assert abs(got["coverage"] - want["coverage"]) <= amb_cover / 600
    assert got["precision"] == np.count_nonzero(details["fake_counts"] >= 1) / 500 and got["density"] == int(details["fake_counts"].sum()) / 1500
    assert got["recall"] == np.count_nonzero(details["real_counts"] >= 1) / 600
    assert got["coverage"] == np.count_nonzero(details["coverage_minima"] <= details["real_radii"]) / 600
    assert 0.0 < got["precision"] <= 1.0 and 0.0 < got["recall"] <= 1.0


def test_the_hand_example_on_the_device():
    from gansynth_amd import manifold, metrics
    from tests.test_knn_cpu import FAKE, REAL
    details = {}
    got = metrics.precision_recall_device(REAL, FAKE, k=1, details=details)
    print(got, {key: value.tolist() for key, value in details.items()})
    assert got == dict(precision=2 / 3, recall=1.0, density=1.0, coverage=3 / 4)
    assert details["real_radii"].tolist() == [1.0, 1.0, 1.0, 64.0] and details["fake_radii"].tolist() == [9.0, 9.0, 272.25]
    assert details["fake_counts"].tolist() == [2, 1, 0] and details["real_counts"].tolist() == [1, 2, 2, 1]
    assert details["coverage_minima"].tolist() == [0.25, 0.25, 2.25, 42.25]
    result = manifold.figures(torch.from_numpy(REAL).cuda(), torch.from_numpy(FAKE).cuda(), 1)
    assert (result.precision, result.recall, result.density, result.coverage) == (2 / 3, 1.0, 1.0, 3 / 4)


# ----------------------------------------------------------------------------------------------------------------- evaluate and the driver
def test_evaluate_with_prd(tmp_path, gpu_store):
    from gansynth_amd import checkpoint, metrics
    from tests.test_classifier_gpu import _classifier_file, _gan
    clf = _classifier_file(tmp_path / "clf.safetensors")
    outs, feats = {}, {}
    for mode in ("plain", "prd"):
        model = _gan(8, 3)                                     # 24 examples per side
        model._ensure_built(torch.randn(8, 256, device="cuda"), torch.eye(61, device="cuda")[:8])
        if mode == "plain":
            checkpoint.save(model, str(tmp_path))
        feats[mode] = {}
        kw = {} if mode == "plain" else dict(prd=True, prd_k=2)
        outs[mode] = model.evaluate(str(tmp_path), None, clf, "images:0", ["features:0", "logits:0"], features_out=feats[mode], **kw)
        print(mode, outs[mode])
    keys = {"precision", "recall", "density", "coverage"}
    assert set(outs["plain"]) == {"frechet_inception_distance"} and set(outs["prd"]) == set(outs["plain"]) | keys
    assert outs["prd"]["frechet_inception_distance"] == outs["plain"]["frechet_inception_distance"]
    assert np.array_equal(feats["prd"]["real_features"], feats["plain"]["real_features"])
    want = metrics.precision_recall_device(feats["prd"]["real_features"], feats["prd"]["fake_features"], k=2)
    assert all(outs["prd"][key] == want[key] for key in keys)                               # bit for bit
    with pytest.raises(ValueError, match="prd=True needs a classifier"):
        model.evaluate(str(tmp_path), None, None, prd=True)
    with pytest.raises(ValueError, match="prd=True needs a classifier"):
        model.evaluate(str(tmp_path), None, None, swd=True, prd=True)
    with pytest.raises(ValueError, match="prd_k must be an integer in"):
        model.evaluate(str(tmp_path), None, clf, prd=True, prd_k=9)


def test_gan_synth_main_prd(tmp_path):
    from tests.test_classifier_gpu import _classifier_file
    clf = _classifier_file(tmp_path / "clf.safetensors", seed=10)
    cmd = [sys.executable, os.path.join(ROOT, "gan_synth_main.py"), "--evaluate", "--synthetic", "--prd", "--classifier", clf,
           "--model_dir", str(tmp_path / "model"), "--batch_size", "8", "--num_generate_batches", "3"]
    r = subprocess.run(cmd, cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    line = [s for s in r.stdout.splitlines() if "frechet_inception_distance" in s][-1]
    print(line)
    assert all(f"'{key}'" in line for key in ("precision", "recall", "density", "coverage")) and "inception_score" not in line
