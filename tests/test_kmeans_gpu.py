"""GPU: gs_kmeans_assign / _update / _mindist element-wise against the float64 restatement (tests/kmeans_ref.py), then kmeans.kmeans,
metrics.num_different_bins_device, GANSynth.evaluate(ndb="device") and the driver's --ndb.  Every figure is printed before it is asserted.

The kernel tests call the C entries themselves: the inputs sit inside NaN-filled buffers with row slack (ldx = d + 3), once 16-byte aligned and
once one float off, every output inside a sentinel-filled buffer, and nothing outside the outputs may change.

Bounds (u = 2^-24): a distance is a fp32 sum of d non-negative terms, each a rounded square of a rounded difference: within (d + 8) u of its
float64 value in any order of summation (kmeans_ref.dist_bound).  A label must be the float64 argmin unless the float64 best and second best
lie within that bound of each other; such rows may be at most 0.1 % of a test's rows.  The inputs are seeded Gaussians with a common offset; on
every one of them the fp32 numpy restatement has no such row at all (checked on the CPU; the tests print the count and hold the cap)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import kmeans_ref as KR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = KR.TILE
PAD = 64                                   # floats of sentinel on either side of every buffer
I_SENT, F_SENT = -7777, -12345.5
# (d, k, n): every d of {1, 3, 65, 512, 513}, k of {1, 2, 50, 64, 65, 256}, n of {1, T - 1, T, T + 1, 2 T + 35}; the edges combined
SHAPES = [(1, 1, 1), (3, 2, T - 1), (65, 50, T), (512, 64, T + 1), (513, 65, 2 * T + 35), (65, 256, 2 * T + 35), (3, 50, 1), (512, 2, T - 1), (1, 256, T + 1),
          (513, 1, T)]


def _lib():
    from gansynth_amd import _lib as L
    return L, L.load()


@functools.lru_cache(maxsize=None)
def _inputs(d, k, n):
    """-> (x [n, d] fp32, centres [k, d] fp32, float64 labels, minima, the distance matrix): seeded by the shape, computed once."""
    rng = np.random.default_rng(1000 * d + 10 * k + n)
    c = (4.0 + 0.7 * rng.standard_normal((k, d))).astype(np.float32)
    x = (c[rng.integers(0, k, n)] + 0.5 * rng.standard_normal((n, d))).astype(np.float32)      # rows around the centres, a common offset of 4
    labels, dist, full = KR.assign(x, c)
    assert not KR.ambiguous(full, d).any() and np.array_equal(KR.assign(x, c, np.float32)[0], labels)   # (the claim of the module docstring)
    for a in (x, c, labels, dist, full):
        a.setflags(write=False)
    return x, c, labels, dist, full


def _place(a, aligned, slack=3):
    """a [n, d] inside a NaN-filled device buffer, rows d + slack apart, the first on 16 bytes or one float off: -> (buffer, view, ldx)."""
    n, d = a.shape
    ldx = d + slack
    off = PAD + (0 if aligned else 1)
    buf = torch.full((off + n * ldx + PAD,), float("nan"), device="cuda")
    view = buf[off:off + n * ldx].view(n, ldx)[:, :d]
    view.copy_(torch.from_numpy(np.array(a)))                 # (a copy: the shared inputs are read-only)
    assert (view.data_ptr() % 16 == 0) == aligned
    return buf, view, ldx


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


def _ws(n, d, k):
    from gansynth_amd import kernels
    L, lib = _lib()
    return kernels._ws(lib.gs_kmeans_workspace_bytes(n, d, k), torch.device("cuda"))


def _assign(xv, ldx, cdev, labels, dist=None, changed=None, inertia=None):
    from gansynth_amd import kernels
    L, lib = _lib()
    n, d = xv.shape
    k = cdev.shape[0]
    ws = _ws(n, d, k)
    L.check(lib.gs_kmeans_assign(xv.data_ptr(), ldx, n, d, cdev.data_ptr(), k, labels.data_ptr(), None if dist is None else dist.data_ptr(),
                                 None if changed is None else changed.data_ptr(), None if inertia is None else inertia.data_ptr(), ws.data_ptr(), ws.numel(),
                                 kernels._stream()), "gs_kmeans_assign")
    torch.cuda.synchronize()


def _inertia(xv, ldx, cdev, labels, inertia):
    from gansynth_amd import kernels
    L, lib = _lib()
    n, d = xv.shape
    k = cdev.shape[0]
    ws = _ws(n, d, k)
    L.check(lib.gs_kmeans_inertia(xv.data_ptr(), ldx, n, d, cdev.data_ptr(), k, labels.data_ptr(), inertia.data_ptr(), ws.data_ptr(), ws.numel(),
                                  kernels._stream()), "gs_kmeans_inertia")
    torch.cuda.synchronize()


def _check_labels(got, want, full, d):
    """The label rule of the module docstring: -> the number of ambiguous rows (at most 0.1 % of the rows)."""
    amb = KR.ambiguous(full, d)
    second = np.argsort(full, axis=1, kind="stable")[:, :2]
    wrong = np.flatnonzero(got != want)
    print(f"    labels: {len(wrong)} differ from the float64 argmin, {int(amb.sum())} ambiguous rows of {len(want)} (cap {0.001 * len(want):.3f})")
    assert amb.sum() <= 0.001 * len(want)
    assert all(amb[i] and got[i] in second[i] for i in wrong)
    return int(amb.sum())


# ----------------------------------------------------------------------------------------------------------------- assign
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "one float off"])
@pytest.mark.parametrize("d,k,n", SHAPES, ids=[f"d{d}-k{k}-n{n}" for d, k, n in SHAPES])
def test_assign(d, k, n, aligned):
    x, c, want, dist64, full = _inputs(d, k, n)
    xbuf, xv, ldx = _place(x, aligned)
    cdev = torch.from_numpy(np.array(c)).cuda()
    lbuf, labels = _out(n, I_SENT, torch.int32, aligned)
    dbuf, dist = _out(n, F_SENT, torch.float32, aligned)
    chbuf, changed = _out(1, I_SENT, torch.int32)
    ibuf, inertia = _out(1, F_SENT, torch.float64)
    before = want.copy()
    before[::3] = (before[::3] + 1) % max(k, 2)              # a third of the rows start on another label (for k = 1: on a label that is none)
    before[1::7] = -1
    labels.copy_(torch.from_numpy(before))
    _assign(xv, ldx, cdev, labels, dist, changed, inertia)
    got, gd = labels.cpu().numpy(), dist.cpu().numpy().astype(np.float64)
    err = np.abs(gd - dist64) / np.maximum(dist64, 1e-300)
    print(f"d {d} k {k} n {n}: worst distance error {err.max():.3g} relative (bound {KR.dist_bound(d):.3g})")
    assert np.isfinite(gd).all() and (np.abs(gd - dist64) <= KR.dist_bound(d) * dist64).all()
    _check_labels(got, want, full, d)
    moved = int(np.count_nonzero(before != got))
    total, own = float(inertia.item()), float(gd.sum())
    print(f"    changed {int(changed.item())} (moved labels {moved}); inertia {total!r} against {dist64.sum()!r}: {abs(total - dist64.sum()) / dist64.sum():.3g} relative; "
          f"against the sum of its own dist: {abs(total - own) / own:.3g}")
    assert int(changed.item()) == moved
    assert abs(total - dist64.sum()) <= KR.dist_bound(d) * dist64.sum()
    assert abs(total - own) <= n * 2.0 ** -52 * own           # the sum of the call's own fp32 minima, in double (two orders of n double additions)
    # gs_kmeans_inertia on those labels: every term and every sum in double -- (d + 8) roundings a term and n a sum, at 2^-53, doubled
    jbuf, exact = _out(1, F_SENT, torch.float64)
    _inertia(xv, ldx, cdev, labels, exact)
    want_exact = float(full[np.arange(n), got].sum())
    print(f"    gs_kmeans_inertia {float(exact.item())!r} against {want_exact!r}: {abs(float(exact.item()) - want_exact) / want_exact:.3g} relative")
    assert abs(float(exact.item()) - want_exact) <= (d + 8 + n) * 2.0 ** -52 * want_exact
    first = float(exact.item())
    _inertia(xv, ldx, cdev, labels, exact)
    assert float(exact.item()) == first and _intact(jbuf, exact, F_SENT)
    assert _intact(lbuf, labels, I_SENT) and _intact(dbuf, dist, F_SENT) and _intact(chbuf, changed, I_SENT) and _intact(ibuf, inertia, F_SENT)
    assert np.isnan(xbuf.cpu().numpy()).sum() == xbuf.numel() - n * d       # the input is as it was

    # a second call: the same bits (and nothing moves any more); without the optional outputs: the same labels
    l2buf, labels2 = _out(n, I_SENT, torch.int32, aligned)
    d2buf, dist2 = _out(n, F_SENT, torch.float32, aligned)
    labels2.copy_(labels)
    _assign(xv, ldx, cdev, labels2, dist2, changed, inertia)
    assert torch.equal(labels2, labels) and torch.equal(dist2, dist) and int(changed.item()) == 0 and float(inertia.item()) == total
    labels2.fill_(I_SENT)
    _assign(xv, ldx, cdev, labels2)
    assert torch.equal(labels2, labels) and _intact(l2buf, labels2, I_SENT)


def test_assign_exact_ties_go_to_the_lowest_index():
    """Distances that are exact in fp32 (an integer grid): duplicated centres and equidistant centres, within a wave's group, across the four
    waves and across rounds (k = 70: 52 centres a round, so the duplicate of centre 5 at 60 sits in the second round)."""
    rng = np.random.default_rng(7)
    for d, k in ((3, 4), (5, 70), (33, 256)):
        n = T + 9
        x = rng.integers(-4, 5, (n, d)).astype(np.float32)
        c = rng.integers(-4, 5, (k, d)).astype(np.float32)
        c[k - 1] = c[0]                                       # duplicates: the last centre of the first ...
        x[0] = c[0]                                           # ... and a row that sits on them: distance 0 twice
        if k > 60:
            c[60] = c[5]                                      # ... and, a round later, of centre 5
            x[1] = c[5]
        c[1] = 20.0                                           # two centres away from the grid, 4 apart in the first column,
        c[2] = c[1]
        c[2, 0] += 4.0
        x[2] = c[1]
        x[2, 0] += 2.0                                        # and a row half way: 4 from both
        want, dist64, full = KR.assign(x, c)
        ties = int(np.count_nonzero((full == dist64[:, None]).sum(axis=1) > 1))
        assert want[0] == 0 and want[2] == 1 and dist64[2] == 4.0 and (k <= 60 or want[1] == 5)
        _, xv, ldx = _place(x, False)
        lbuf, labels = _out(n, I_SENT, torch.int32)
        dbuf, dist = _out(n, F_SENT, torch.float32)
        _assign(xv, ldx, torch.from_numpy(np.array(c)).cuda(), labels, dist)
        print(f"d {d} k {k}: {ties} rows with an exact tie; labels equal {np.array_equal(labels.cpu().numpy(), want)}")
        assert ties >= 2
        assert np.array_equal(labels.cpu().numpy(), want)
        assert np.array_equal(dist.cpu().numpy().astype(np.float64), dist64)      # exact: every term is a small integer


# ----------------------------------------------------------------------------------------------------------------- update
def _update(xv, ldx, labels, centres, counts):
    from gansynth_amd import kernels
    L, lib = _lib()
    n, d = xv.shape
    k = centres.shape[0]
    ws = _ws(n, d, k)
    L.check(lib.gs_kmeans_update(xv.data_ptr(), ldx, n, d, labels.data_ptr(), k, centres.data_ptr(), counts.data_ptr(), ws.data_ptr(), ws.numel(),
                                 kernels._stream()), "gs_kmeans_update")
    torch.cuda.synchronize()


def _label_sets(k, n, own):
    """The kernel's own labels, one cluster holding every row, and an adversarial order (all of one cluster first, some clusters empty)."""
    rng = np.random.default_rng(k + n)
    sets = {"the kernel's own": own, "one cluster holds every row": np.full(n, k // 2, dtype=np.int32)}
    sets["sorted, with empty clusters"] = np.sort(rng.integers(0, max(1, k - k // 3), n)).astype(np.int32)
    return sets


@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "one float off"])
@pytest.mark.parametrize("d,k,n", SHAPES, ids=[f"d{d}-k{k}-n{n}" for d, k, n in SHAPES])
def test_update(d, k, n, aligned):
    x, c, _, _, _ = _inputs(d, k, n)
    xbuf, xv, ldx = _place(x, aligned)
    own = torch.empty(n, dtype=torch.int32, device="cuda")
    _assign(xv, ldx, torch.from_numpy(np.array(c)).cuda(), own)
    x64 = x.astype(np.float64)
    for name, labels in _label_sets(k, n, own.cpu().numpy()).items():
        ldev = torch.from_numpy(labels).cuda()
        cbuf, centres = _out(k * d, F_SENT, torch.float32, aligned)
        centres.fill_(F_SENT + 1.0)                            # an empty cluster's centre must keep this
        nbuf, counts = _out(k, I_SENT, torch.int32)
        _update(xv, ldx, ldev, centres.view(k, d), counts)
        got_c, got_n = centres.view(k, d).cpu().numpy().astype(np.float64), counts.cpu().numpy()
        want_n = np.bincount(labels, minlength=k)
        worst = 0.0
        for kk in range(k):
            if want_n[kk] == 0:
                assert (got_c[kk] == F_SENT + 1.0).all(), (name, kk)
                continue
            rows = x64[labels == kk]
            m = len(rows)
            err, bound = np.abs(got_c[kk] - rows.mean(axis=0)), (m + 2) * KR.U * np.abs(rows).sum(axis=0) / m
            worst = max(worst, float((err / bound).max()))
            assert (err <= bound).all(), (name, kk, m)
        print(f"d {d} k {k} n {n}, {name}: {int((want_n == 0).sum())} empty clusters, worst centre error {worst:.3g} of its bound")
        assert np.array_equal(got_n, want_n)
        assert _intact(cbuf, centres, F_SENT) and _intact(nbuf, counts, I_SENT)
        c2buf, centres2 = _out(k * d, F_SENT, torch.float32, aligned)
        centres2.fill_(F_SENT + 1.0)
        _update(xv, ldx, ldev, centres2.view(k, d), counts)
        assert torch.equal(centres2, centres)                  # bit-identical
    assert np.isnan(xbuf.cpu().numpy()).sum() == xbuf.numel() - n * d


# ----------------------------------------------------------------------------------------------------------------- mindist
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "one float off"])
@pytest.mark.parametrize("d,k,n", SHAPES[:5], ids=[f"d{d}-n{n}" for d, _, n in SHAPES[:5]])
def test_mindist(d, k, n, aligned):
    from gansynth_amd import kernels
    L, lib = _lib()
    x = _inputs(d, k, n)[0]
    _, xv, ldx = _place(x, aligned)
    pick = [0, n // 2]
    dbuf, dist = _out(n, F_SENT, torch.float32, aligned)
    want = None
    for step, row in enumerate(pick):
        centre = torch.from_numpy(x[row].copy()).cuda()
        L.check(lib.gs_kmeans_mindist(xv.data_ptr(), ldx, n, d, centre.data_ptr(), dist.data_ptr(), 1 if step == 0 else 0, kernels._stream()), "gs_kmeans_mindist")
        new = KR.sqdist(x, x[row][None])[:, 0]
        want = new if want is None else np.minimum(want, new)
        got = dist.cpu().numpy().astype(np.float64)
        err = np.abs(got - want) / np.maximum(want, 1e-300)
        print(f"d {d} n {n} step {step}: worst error {np.where(want > 0, err, 0).max():.3g} relative (bound {KR.dist_bound(d):.3g}); zeros at {np.flatnonzero(got == 0).tolist()[:4]}")
        assert (np.abs(got - want) <= KR.dist_bound(d) * want).all()
        assert got[row] == 0.0 and _intact(dbuf, dist, F_SENT)
        again = dist.clone()
        L.check(lib.gs_kmeans_mindist(xv.data_ptr(), ldx, n, d, centre.data_ptr(), again.data_ptr(), 1 if step == 0 else 0, kernels._stream()), "gs_kmeans_mindist")
        assert torch.equal(again, dist)
    # the Python layer: the same numbers from a view with row slack
    first = kernels.kmeans_mindist(xv, torch.from_numpy(x[pick[0]].copy()).cuda())
    both = kernels.kmeans_mindist(xv, torch.from_numpy(x[pick[1]].copy()).cuda(), first)
    assert both is first and torch.equal(both, dist)


def test_python_layer_matches_the_entries():
    from gansynth_amd import kernels
    d, k, n = 65, 50, T
    x, c, want, dist64, full = _inputs(d, k, n)
    _, xv, ldx = _place(x, False)
    cdev = torch.from_numpy(np.array(c)).cuda()
    labels, dist, changed, inertia = kernels.kmeans_assign(xv, cdev, want_inertia=True)
    assert changed is None and labels.dtype == torch.int32 and inertia.dtype == torch.float64
    _check_labels(labels.cpu().numpy(), want, full, d)
    same, _, changed, none = kernels.kmeans_assign(torch.from_numpy(np.array(x)).cuda(), cdev, labels=labels, want_dist=False)
    assert same is labels and int(changed.item()) == 0 and none is None
    centres = cdev.clone()
    exact = kernels.kmeans_inertia(xv, cdev, labels)
    assert exact.dtype == torch.float64 and abs(float(exact.item()) - float(inertia.item())) <= KR.dist_bound(d) * float(exact.item())
    counts = kernels.kmeans_update(xv, labels, centres)
    assert np.array_equal(counts.cpu().numpy(), np.bincount(labels.cpu().numpy(), minlength=k))
    with pytest.raises(ValueError, match="x must be on the HIP device"):
        kernels.kmeans_assign(torch.from_numpy(np.array(x)), cdev)
    with pytest.raises(ValueError, match="centres is on cpu"):
        kernels.kmeans_assign(xv, torch.from_numpy(np.array(c)))


# ----------------------------------------------------------------------------------------------------------------- the algorithm
@pytest.mark.parametrize("name", list(KR.CASES))
def test_kmeans_from_a_given_init(name):
    """Iterations equal the float64 restatement's, labels differ on at most 0.1 % of the rows (the fp32 restatement: on none, printed), and the
    inertia's relative error is within 4 times the fp32 restatement's (on the CPU: 6.0e-9, 7.1e-9, 9.5e-9, 1.3e-10 for the four cases)."""
    from gansynth_amd import kmeans
    x, init = KR.case(name)
    k = KR.CASES[name][2]
    labels64, inertia64, iterations64, centres64 = KR.case_lloyd(name)
    labels32, inertia32, iterations32, _ = KR.case_lloyd(name, True)
    got = kmeans.kmeans(x, k, init=init)
    differ = int(np.count_nonzero(got.labels.cpu().numpy() != labels64))
    mine, single = abs(got.inertia - inertia64) / inertia64, abs(inertia32 - inertia64) / inertia64
    print(f"{name}: iterations {got.iterations} (float64 {iterations64}, fp32 restatement {iterations32}); labels differ on {differ} rows "
          f"(fp32 restatement {int(np.count_nonzero(labels32 != labels64))}); inertia {got.inertia!r} against {inertia64!r}: {mine:.3g} relative "
          f"(fp32 restatement {single:.3g})")
    assert got.run == 0 and got.seed_rows is None
    assert got.iterations == iterations64
    assert differ <= 0.001 * len(x)
    assert np.array_equal(got.counts, np.bincount(got.labels.cpu().numpy(), minlength=k))
    assert mine <= 4.0 * single


SEEDED = [("3000x16x10", 0, 4), ("2049x65x7", 0, 4)]


@pytest.mark.parametrize("name,seed,n_init", SEEDED, ids=[s[0] for s in SEEDED])
def test_kmeans_seeded(name, seed, n_init):
    """Seeds 0 .. 5 of both inputs: the fp32 restatement picks the float64 restatement's rows in every one of them (checked on the CPU), so the
    device must.  Best run: the restatement's (run 1 for both; for 2049x65x7 runs 1 and 2 reach the same partition and the same inertia to
    the bit -- the lowest index wins -- and for 3000x16x10 the runner-up is 8.7e-7 away, a hundred times the rounding).  Inertia: labels agree,
    so it differs by the rounding of the distances, (d + 8) u, and to second order by that of the means."""
    from gansynth_amd import kmeans
    x, _ = KR.case(name)
    n, d, k, _ = KR.CASES[name]
    xdev = kmeans.to_device(x)
    for stream in range(seed, seed + 6):
        rows = kmeans.seed_rows(xdev, k, np.random.Generator(np.random.PCG64(stream)))
        want = KR.seed_rows(x, k, stream)
        print(f"{name} stream {stream}: rows {rows}")
        assert rows == want
    ref = KR.kmeans(x, k, seed=seed, n_init=n_init)
    got = kmeans.kmeans(x, k, seed=seed, n_init=n_init)
    rel = abs(got.inertia - ref["inertia"]) / ref["inertia"]
    print(f"{name}: best run {got.run} (restatement {ref['run']}, inertias {ref['inertias']}), inertia {got.inertia!r} against {ref['inertia']!r}: {rel:.3g}")
    assert got.run == ref["run"] and got.seed_rows == ref["seed_rows"] and got.iterations == ref["iterations"]
    assert rel <= KR.dist_bound(d)


def test_kmeans_relocates_an_empty_cluster():
    from gansynth_amd import kmeans
    x, init = KR.case("3000x16x10")
    init = init.copy()
    init[3] = 1000.0                                           # far from all data: empty after the first assign
    log = []
    labels64, _, iterations64, _ = KR.lloyd(x, init, 300, log=log)
    (cluster, row), = log[0]
    one = kmeans.kmeans(x, 10, init=init, max_iter=1)         # one update, the relocation, the closing assign
    print(f"restatement: cluster {cluster} takes row {row}; device centre equals that row: {np.array_equal(one.centres[cluster].cpu().numpy(), x[row])}")
    assert cluster == 3 and np.array_equal(one.centres[3].cpu().numpy(), x[row])
    full = kmeans.kmeans(x, 10, init=init)
    print(f"final counts {full.counts.tolist()}, iterations {full.iterations} (restatement {iterations64})")
    assert (full.counts > 0).all() and full.iterations == iterations64
    assert np.count_nonzero(full.labels.cpu().numpy() != labels64) <= 0.001 * len(x)


def test_kmeans_max_iter_1_returns_the_assignment_to_its_centres():
    from gansynth_amd import kernels, kmeans
    x, init = KR.case("2049x65x7")
    got = kmeans.kmeans(x, 7, init=init, max_iter=1)
    labels = kernels.kmeans_assign(kmeans.to_device(x), got.centres)[0]
    assert got.iterations == 1 and torch.equal(labels, got.labels)
    assert float(kernels.kmeans_inertia(kmeans.to_device(x), got.centres, got.labels).item()) == got.inertia
    none = kmeans.kmeans(x, 7, init=init, max_iter=0)          # no update at all: the assignment to init
    assert none.iterations == 0 and np.array_equal(none.centres.cpu().numpy(), init)
    assert np.array_equal(none.labels.cpu().numpy(), KR.assign(x, init)[0])


# ----------------------------------------------------------------------------------------------------------------- NDB
def test_ndb_of_a_set_against_itself_and_against_a_shifted_copy():
    from gansynth_amd import metrics
    x, _ = KR.mixture(1500, 16, 6, 1.0, 21)
    details = {}
    assert metrics.num_different_bins_device(x, x, num_bins=10, n_init=2, details=details) == 0
    assert details["jsd"] == 0.0 and np.array_equal(details["real_counts"], details["fake_counts"]) and details["real_counts"].sum() == 1500
    assert metrics.num_different_bins_device(x, x) == 0      # the defaults: 50 bins, ten restarts
    shifted = metrics.num_different_bins_device(x, x + np.float32(3.0), num_bins=10, n_init=2, details=details)
    print(f"x against x + 3: {shifted} of 10 bins differ, jsd {details['jsd']:.4f}")
    assert shifted > 0 and 0.0 < details["jsd"] <= np.log(2.0)


@pytest.mark.parametrize("seed,n_real,n_fake", [(11, 1200, 1200), (12, 1500, 700)])
def test_ndb_equals_the_restatement(seed, n_real, n_fake):
    """Two seeded feature sets on which the fp32 restatement gives the float64 restatement's rows, counts and NDB (checked on the CPU: 8 and 6)."""
    from gansynth_amd import metrics
    real, _ = KR.mixture(n_real, 16, 6, 1.0, seed)
    fake, _ = KR.mixture(n_fake, 16, 6, 1.0, seed + 100)
    fake = fake + np.float32(0.15)
    want, ref = KR.ndb(real, fake, num_bins=10, seed=3, n_init=3)
    details = {}
    got = metrics.num_different_bins_device(torch.from_numpy(real), fake, num_bins=10, seed=3, n_init=3, details=details)
    print(f"NDB {got} (restatement {want}); jsd {details['jsd']!r} (restatement {ref['jsd']!r}); inertia {details['inertia']!r} ({ref['inertia']!r})")
    assert got == want
    assert np.array_equal(details["real_counts"], ref["real_counts"]) and np.array_equal(details["fake_counts"], ref["fake_counts"])
    assert abs(details["jsd"] - ref["jsd"]) <= 1e-12


# ----------------------------------------------------------------------------------------------------------------- evaluate
def test_evaluate_with_ndb_on_the_device(tmp_path, gpu_store, monkeypatch):
    """The reduced model of tests/test_classifier_gpu.py, scikit-learn hidden: the default call returns the three figures it returned (and drops
    NDB silently), ndb="device" adds num_different_bins and bin_jsd to the same three."""
    from gansynth_amd import checkpoint, metrics
    from tests.test_classifier_gpu import _classifier_file, _gan
    monkeypatch.setitem(sys.modules, "sklearn", None)
    clf = _classifier_file(tmp_path / "clf.safetensors")
    outs, feats = {}, {}
    for mode in ("sklearn", "device"):
        model = _gan(16, 36)                                   # 576 examples per side
        model._ensure_built(torch.randn(16, 256, device="cuda"), torch.eye(61, device="cuda")[:16])
        if mode == "sklearn":
            checkpoint.save(model, str(tmp_path))
        feats[mode] = {}
        kw = {} if mode == "sklearn" else dict(ndb="device")
        outs[mode] = model.evaluate(str(tmp_path), None, clf, "images:0", ["features:0", "logits:0"], features_out=feats[mode], extra_metrics=True, **kw)
        print(mode, outs[mode])
    f = feats["sklearn"]
    want = dict(frechet_inception_distance=metrics.frechet_inception_distance(f["real_features"], f["fake_features"]),
                inception_score=metrics.inception_score(f["fake_logits"]),
                pitch_accuracy=float(np.mean(np.argmax(f["fake_logits"], axis=1) == np.argmax(f["labels"], axis=1))))
    assert outs["sklearn"] == want                             # exactly the keys and values of before
    assert np.array_equal(feats["device"]["real_features"], f["real_features"]) and np.array_equal(feats["device"]["fake_features"], f["fake_features"])
    assert set(outs["device"]) == set(want) | {"num_different_bins", "bin_jsd"}
    assert all(outs["device"][key] == want[key] for key in want)
    details = {}
    assert outs["device"]["num_different_bins"] == metrics.num_different_bins_device(f["real_features"], f["fake_features"], details=details)
    assert outs["device"]["bin_jsd"] == details["jsd"] and 0 <= outs["device"]["num_different_bins"] <= 50
    with pytest.raises(ValueError, match="ndb must be"):
        model.evaluate(str(tmp_path), None, clf, ndb="host")


def test_gan_synth_main_ndb(tmp_path):
    from tests.test_classifier_gpu import _classifier_file
    clf = _classifier_file(tmp_path / "clf.safetensors", seed=10)
    cmd = [sys.executable, os.path.join(ROOT, "gan_synth_main.py"), "--evaluate", "--synthetic", "--ndb", "--classifier", clf,
           "--model_dir", str(tmp_path / "model"), "--batch_size", "16", "--num_generate_batches", "36"]
    r = subprocess.run(cmd, cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    line = [s for s in r.stdout.splitlines() if "frechet_inception_distance" in s][-1]
    print(line)
    assert "'num_different_bins'" in line and "'bin_jsd'" in line and "'inception_score'" in line
