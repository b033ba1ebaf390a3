"""GPU: gs_kid_sums against the longdouble restatement (tests/kid_ref.py), then kernels.kid_sums, kid.figures, metrics.kernel_inception_distance_
device, GANSynth.evaluate(kid=True) and the driver's --kid.  Every figure is printed before it is asserted.

The kernel tests call the C entry itself: the inputs sit inside NaN-filled buffers with row slack (ld = d + 3), once 16-byte aligned and once
one float off, `out` and `ws` inside sentinel-filled buffers, and nothing outside them may change.

The bound for each of the three sums, from counted roundings, not measured (u = 2^-53, B = sum over the pairs of (sum_c |x_c y_c| / d + 1)^3):

    |S_dev - S_ref| <= u (3 d + 8 + L) B.

A product of two fp32 features is exact in fp64, so the dot carries at most d roundings, those of its additions, each at most u of
sum_c |x_c y_c|; t = p / d + 1 adds two and the cube two.  With s = sum_c |x_c y_c| / d + 1 a relative error e of t's ingredients moves
k = t^3 by at most 3 s^2 (s e): d + 2 roundings through the cube and 2 of the cube itself are (3 (d + 2) + 2) u s^3 = (3 d + 8) u s^3 a pair.
Every k is positive, so an addition's rounding is at most u of what the whole sum will be, and a term goes through at most L additions, the
longest chain of the summation order:

    L = 63 + 8 + 0 + 8 = 79:  a lane adds its 64 values in one chain (63 additions), the block's 256 lanes meet in a tree of depth 8, a fold
    thread adds ceil(tiles / 256) partials (every job here has at most 64 tiles: one partial, no addition) and the fold's 256 threads meet in
    the same tree.  (The doubling of an off-diagonal tile's partial is exact.)

Checked on the CPU for all seven shapes: numpy float64 lands at <= 0.05 of the bound on every sum, an fp32 restatement exceeds it by 7e4 to 4e7;
one pair is at least 1e-6 of a sum and the bound below 1e-12 of it, so the bound admits a correct kernel and rejects any lower-precision
shortcut and any lost, doubled or diagonal pair.  No exception rule, no share of cases left out."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import kid_ref as DR
from tests import knn_ref as NR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD = 64                                   # elements of sentinel on either side of every buffer
D_SENT = -12345.5
CHAIN = 79                                 # L of the module docstring
# (d, n, m): every d residue mod 4, a d past the chunk of 32 by one, sides below, at and past one tile of 128 and past two and four, a diagonal
# tile that is partly empty
SHAPES = [(1, 2, 2), (3, 255, 257), (4, 1024, 1024), (65, 256, 300), (512, 257, 64), (513, 547, 291), (512, 5, 547)]
IDS = [f"d{d}-n{n}-m{m}" for d, n, m in SHAPES]
NAMES = ("Sxx", "Syy", "Sxy")


def _lib():
    from gansynth_amd import _lib as L
    return L, L.load()


@functools.lru_cache(maxsize=None)
def _inputs(d, n, m):
    """-> (x [n, d], y [m, d]) fp32, read-only: seeded by the shape, rows around 8 shared centres (as test_knn_gpu._inputs)."""
    rng = np.random.default_rng(100000 * d + 100 * n + m)
    a, centres = NR.clustered(n, d, rng)
    b, _ = NR.clustered(m, d, rng, centres)
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


@functools.lru_cache(maxsize=None)
def _features():
    """Feature-like rows, |N(0.5, 0.2)|: -> (real [300, 512], fake of the same distribution [280, 512]), read-only."""
    rng = np.random.default_rng(512)
    real, fake = (np.abs(rng.normal(0.5, 0.2, (rows, 512))).astype(np.float32) for rows in (300, 280))
    real.setflags(write=False)
    fake.setflags(write=False)
    return real, fake


@functools.lru_cache(maxsize=None)
def _want(d, n, m):
    x, y = _inputs(d, n, m)
    return DR.three_sums(x, y)


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


def _sums(xv, ldx, yv, ldy, xi=None, yi=None, out_aligned=True):
    """gs_kid_sums on views: -> [S, 3] float64 (numpy); out and ws sit between sentinels, which must survive."""
    from gansynth_amd import kernels
    L, lib = _lib()
    (n, d), m = xv.shape, yv.shape[0]
    subsets, size = (0, 0) if xi is None else tuple(xi.shape)
    nbytes = int(lib.gs_kid_workspace_bytes(n, m, d, subsets, size))
    assert nbytes >= 16 and nbytes % 16 == 0
    wbuf, ws = _out(nbytes // 8, D_SENT, torch.float64)
    obuf, out = _out(3 * max(subsets, 1), D_SENT, torch.float64, out_aligned)
    assert ws.data_ptr() % 16 == 0
    L.check(lib.gs_kid_sums(xv.data_ptr(), ldx, n, yv.data_ptr(), ldy, m, d, None if xi is None else xi.data_ptr(), None if yi is None else yi.data_ptr(),
                            subsets, size, out.data_ptr(), ws.data_ptr(), nbytes, kernels._stream()), "gs_kid_sums")
    torch.cuda.synchronize()
    assert _intact(obuf, out, D_SENT) and _intact(wbuf, ws, D_SENT)
    return out.view(-1, 3).cpu().numpy()


def _check(got, want, terms, d, what):
    """The three sums of one set pair against the restatement and the docstring's bound."""
    bound = DR.sum_bound(d, CHAIN, terms)
    err = np.abs(got.astype(DR.LD) - want).astype(np.float64)
    for name, g, w, e, b in zip(NAMES, got, want, err, bound):
        print(f"{what} {name}: device {g!r}, restatement {float(w)!r}, error {e:.3g} = {e / b:.3g} of the bound {b:.3g} ({b / float(w):.3g} of the sum)")
    assert np.isfinite(got).all() and (err <= bound).all()


# ----------------------------------------------------------------------------------------------------------------- the full sets
@pytest.mark.parametrize("d,n,m", SHAPES, ids=IDS)
def test_full_sums(d, n, m):
    x, y = _inputs(d, n, m)
    want, terms = _want(d, n, m)
    results = {}
    for aligned in (True, False):
        xbuf, xv, ldx = _place(x, aligned)
        ybuf, yv, ldy = _place(y, aligned)
        got = _sums(xv, ldx, yv, ldy, out_aligned=aligned)
        assert got.shape == (1, 3)
        _check(got[0], want, terms, d, f"d {d} n {n} m {m} {'aligned' if aligned else 'one float off'}")
        assert np.array_equal(_sums(xv, ldx, yv, ldy, out_aligned=aligned), got)               # two calls: the same bits
        assert np.isnan(xbuf.cpu().numpy()).sum() == xbuf.numel() - n * d and np.isnan(ybuf.cpu().numpy()).sum() == ybuf.numel() - m * d
        results[aligned] = got
    assert np.array_equal(results[True], results[False])                                       # the two placements: the same bits
    # the roles exchanged: the same pairs, Sxx and Syy change places (another tiling of Sxy: within the bound, not the same bits)
    _, xv, ldx = _place(x, True)
    _, yv, ldy = _place(y, False)
    swapped = _sums(yv, ldy, xv, ldx)[0]
    assert swapped[0] == results[True][0, 1] and swapped[1] == results[True][0, 0]
    _check(swapped, want[[1, 0, 2]], terms[[1, 0, 2]], d, f"d {d} n {n} m {m} exchanged")


def test_the_hand_example_on_the_device():
    """d = 1, x = {1, 2}, y = {0, 3}: every number is a small integer, the sums are exact: 54, 2, 409 and KID = -176.5."""
    from gansynth_amd import kid, metrics
    x, y = np.array([[1.0], [2.0]], dtype=np.float32), np.array([[0.0], [3.0]], dtype=np.float32)
    _, xv, ldx = _place(x, False)
    _, yv, ldy = _place(y, True)
    got = _sums(xv, ldx, yv, ldy)
    print(got)
    assert got.tolist() == [[54.0, 2.0, 409.0]] and kid.estimate(got[0], 2, 2) == -176.5
    out = metrics.kernel_inception_distance_device(x, y, subsets=2)
    print(out)
    assert out == dict(kernel_inception_distance=-176.5, kernel_inception_distance_subset_mean=-176.5, kernel_inception_distance_subset_std=0.0)


def test_a_duplicate_row_is_a_pair_like_any_other():
    """Row 3 repeated at row 200 (another tile) and in y: only the index excludes.  Against the restatement, which excludes by index too."""
    x, y = (np.array(t) for t in _inputs(65, 256, 300))
    x[200] = x[3]
    y[17] = x[3]
    want, terms = DR.three_sums(x, y)
    _, xv, ldx = _place(x, False)
    _, yv, ldy = _place(y, True)
    _check(_sums(xv, ldx, yv, ldy)[0], want, terms, 65, "duplicates")


# ----------------------------------------------------------------------------------------------------------------- subsets
@pytest.mark.parametrize("size", [100, 257])
def test_subsets(size):
    """Three subsets of the 547 x 291 inputs, found through the index lists: subsets 0 and 1 overlap (the same rows in two subsets), 2 is drawn
    apart.  Each of the 9 sums is within its bound of the restatement on the gathered rows, bit-equal to the same subset run alone and to a
    second call."""
    d, n, m = 513, 547, 291
    x, y = _inputs(d, n, m)
    rng = np.random.default_rng(size)
    px, py, qx, qy = rng.permutation(n), rng.permutation(m), rng.permutation(n), rng.permutation(m)
    xi = np.stack([px[:size], px[size // 2:size // 2 + size], qx[:size]]).astype(np.int32)
    yi = np.stack([py[:size], py[17:17 + size], qy[:size]]).astype(np.int32)
    assert len(set(xi[0]) & set(xi[1])) >= size // 2 - 1 and len(set(yi[0]) & set(yi[1])) >= size - 17
    xbuf, xv, ldx = _place(x, False)
    ybuf, yv, ldy = _place(y, True)
    xd, yd = torch.from_numpy(xi).cuda(), torch.from_numpy(yi).cuda()
    got = _sums(xv, ldx, yv, ldy, xd, yd)
    assert got.shape == (3, 3)
    for s in range(3):
        want, terms = DR.three_sums(x[xi[s]], y[yi[s]])
        _check(got[s], want, terms, d, f"size {size} subset {s}")
        alone = _sums(xv, ldx, yv, ldy, xd[s:s + 1].contiguous(), yd[s:s + 1].contiguous())
        assert np.array_equal(alone[0], got[s])                                                # alone or as entry s of the batch: the same bits
    assert np.array_equal(_sums(xv, ldx, yv, ldy, xd, yd, out_aligned=False), got)             # a second call: the same bits
    assert np.isnan(xbuf.cpu().numpy()).sum() == xbuf.numel() - n * d and np.isnan(ybuf.cpu().numpy()).sum() == ybuf.numel() - m * d


# ----------------------------------------------------------------------------------------------------------------- feature-like inputs
@pytest.mark.parametrize("shift", [0.0, 0.05])
def test_feature_like_inputs(shift):
    """300 x 280 x 512 rows of |N(0.5, 0.2)|, both sets from one distribution and with the fake side shifted by 0.05: the three means agree to
    three or four digits, and the full-set KID is within the bound that the three sums' bounds imply for it."""
    from gansynth_amd import kid
    real, fake = _features()
    fake = fake + np.float32(shift)
    n, m, d = 300, 280, 512
    want, terms = DR.three_sums(real, fake)
    _, xv, ldx = _place(real, True)
    _, yv, ldy = _place(fake, False)
    got = _sums(xv, ldx, yv, ldy)[0]
    _check(got, want, terms, d, f"features, shift {shift}")
    value, ref = kid.estimate(got, n, m), DR.estimate(want, n, m)
    bound = DR.estimate_bound(DR.sum_bound(d, CHAIN, terms), want, n, m)
    means = (float(want[0]) / (n * (n - 1)), float(want[1]) / (m * (m - 1)), float(want[2]) / (n * m))
    print(f"shift {shift}: the three means {means}; KID device {value!r}, restatement {float(ref)!r}, error {abs(float(value - ref)):.3g}, bound {bound:.3g}")
    assert abs(float(value - ref)) <= bound
    if shift:
        assert value > 0 and value > 1e6 * bound


# ----------------------------------------------------------------------------------------------------------------- the Python layers
def test_python_layers_against_the_restatement():
    """kernels.kid_sums gives the entry's bits; kid.figures and metrics.kernel_inception_distance_device follow kid_ref.figures on the same draws:
    every subset's estimate within the bound its sums imply, the mean within the mean of those bounds and the standard deviation within their
    maximum (|std(a) - std(b)| <= max |a - b|), each plus the host's own float64 roundings of a mean or a deviation over S values, (S + 8) u of
    the largest estimate."""
    from gansynth_amd import kernels, kid, metrics
    real, fake = _features()
    fake = fake + np.float32(0.05)
    n, m, d, S, size, seed = 300, 280, 512, 5, 100, 3
    want = DR.figures(real, fake, S, size, seed)
    _, xv, ldx = _place(real, False)
    _, yv, ldy = _place(fake, True)
    xi, yi = kid.draw_subsets(n, m, S, size, seed)
    assert np.array_equal(xi, DR.draw_subsets(n, m, S, size, seed)[0]) and np.array_equal(yi, DR.draw_subsets(n, m, S, size, seed)[1])
    full = kernels.kid_sums(xv, yv)                                                            # views with row slack are taken as they stand
    assert full.dtype == torch.float64 and full.is_cuda and np.array_equal(full.cpu().numpy(), _sums(xv, ldx, yv, ldy))
    batch = kernels.kid_sums(xv, yv, xi, torch.from_numpy(yi.astype(np.int64)).cuda())        # lists from the host or the device, int32 or int64
    assert np.array_equal(batch.cpu().numpy(), _sums(xv, ldx, yv, ldy, torch.from_numpy(xi).cuda(), torch.from_numpy(yi).cuda()))
    with pytest.raises(ValueError, match="x must be on the HIP device"):
        kernels.kid_sums(torch.from_numpy(np.array(real)), yv)
    with pytest.raises(ValueError, match="y is on cpu"):
        kernels.kid_sums(xv, torch.from_numpy(np.array(fake)))
    with pytest.raises(ValueError, match="yi holds an index outside its set of 280 rows \\(280\\)"):
        kernels.kid_sums(xv, yv, torch.from_numpy(xi).cuda(), torch.from_numpy(yi).cuda() + int(m - yi.max()))

    result = kid.figures(xv, yv, S, size, seed)
    details = {}
    got = metrics.kernel_inception_distance_device(real, torch.from_numpy(np.array(fake)), subsets=S, subset_size=size, seed=seed, details=details)
    assert np.array_equal(result.sums, full.cpu().numpy()[0]) and np.array_equal(result.subset_sums, batch.cpu().numpy()) and result.size == size
    assert set(got) == {"kernel_inception_distance", "kernel_inception_distance_subset_mean", "kernel_inception_distance_subset_std"}
    assert all(isinstance(v, float) for v in got.values())
    assert (got["kernel_inception_distance"], got["kernel_inception_distance_subset_mean"], got["kernel_inception_distance_subset_std"]) == \
        (result.kid, result.subset_mean, result.subset_std)
    assert np.array_equal(details["subset_kids"], result.subset_kids) and np.array_equal(details["sums"], result.sums) and details["size"] == size
    full_bound = DR.estimate_bound(DR.sum_bound(d, CHAIN, want["sum_terms"]), want["sums"], n, m)
    sub_bounds = DR.estimate_bound(DR.sum_bound(d, CHAIN, want["subset_sum_terms"]), want["subset_sums"], size, size)
    host = (S + 8) * DR.U * float(np.abs(want["subset_kids"]).max())
    print(f"KID {result.kid!r} (restatement {want['kid']!r}, bound {full_bound:.3g}); subsets {result.subset_kids.tolist()} (restatement "
          f"{want['subset_kids'].tolist()}, bounds {sub_bounds.tolist()}); mean {result.subset_mean!r} ({want['subset_mean']!r}), std {result.subset_std!r} "
          f"({want['subset_std']!r}), host roundings {host:.3g}")
    assert abs(result.kid - want["kid"]) <= full_bound + DR.U * abs(want["kid"])               # (the restatement's cast to float64)
    assert (np.abs(result.subset_kids - want["subset_kids"]) <= sub_bounds + DR.U * np.abs(want["subset_kids"])).all()   # (the restatement's cast to float64)
    assert abs(result.subset_mean - want["subset_mean"]) <= sub_bounds.mean() + host
    assert abs(result.subset_std - want["subset_std"]) <= sub_bounds.max() + host
    assert result.subset_std > 0 and result.kid > 0
    none = kid.figures(xv, yv, 0, size, seed)                                                  # no subsets: the full figure alone
    assert none.kid == result.kid and np.isnan(none.subset_mean) and np.isnan(none.subset_std) and none.subset_kids.shape == (0,)


# ----------------------------------------------------------------------------------------------------------------- evaluate and the driver
def test_evaluate_with_kid(tmp_path, gpu_store):
    from gansynth_amd import checkpoint
    from tests.test_classifier_gpu import _classifier_file, _gan
    clf = _classifier_file(tmp_path / "clf.safetensors")
    outs, feats = {}, {}
    for mode in ("plain", "kid"):
        model = _gan(8, 3)                                     # 24 examples per side
        model._ensure_built(torch.randn(8, 256, device="cuda"), torch.eye(61, device="cuda")[:8])
        if mode == "plain":
            checkpoint.save(model, str(tmp_path))
        feats[mode] = {}
        kw = {} if mode == "plain" else dict(kid=True, kid_subsets=4, kid_subset_size=16, kid_seed=5)
        outs[mode] = model.evaluate(str(tmp_path), None, clf, "images:0", ["features:0", "logits:0"], features_out=feats[mode], **kw)
        print(mode, outs[mode])
    keys = ("kernel_inception_distance", "kernel_inception_distance_subset_mean", "kernel_inception_distance_subset_std")
    assert set(outs["plain"]) == {"frechet_inception_distance"} and set(outs["kid"]) == set(outs["plain"]) | set(keys)
    assert outs["kid"]["frechet_inception_distance"] == outs["plain"]["frechet_inception_distance"]   # every other key: unchanged
    assert set(feats["kid"]) == set(feats["plain"]) | {"kid_subset_values"}
    assert all(np.array_equal(feats["kid"][key], feats["plain"][key]) for key in feats["plain"])
    real, fake = feats["kid"]["real_features"], feats["kid"]["fake_features"]
    n, m, d = real.shape[0], fake.shape[0], real.shape[1]
    want = DR.figures(real, fake, 4, 16, 5)
    full_bound = DR.estimate_bound(DR.sum_bound(d, CHAIN, want["sum_terms"]), want["sums"], n, m)
    sub_bounds = DR.estimate_bound(DR.sum_bound(d, CHAIN, want["subset_sum_terms"]), want["subset_sums"], 16, 16)
    host = (4 + 8) * DR.U * float(np.abs(want["subset_kids"]).max())
    print(f"{n} x {m} x {d}: restatement {want['kid']!r}, {want['subset_mean']!r}, {want['subset_std']!r}; bounds {full_bound:.3g}, {sub_bounds.tolist()}, host {host:.3g}")
    assert (n, m) == (24, 24) and want["size"] == 16 and feats["kid"]["kid_subset_values"].shape == (4,)
    assert abs(outs["kid"][keys[0]] - want["kid"]) <= full_bound + DR.U * abs(want["kid"])     # (the restatement's cast to float64)
    assert (np.abs(feats["kid"]["kid_subset_values"] - want["subset_kids"]) <= sub_bounds + DR.U * np.abs(want["subset_kids"])).all()
    assert abs(outs["kid"][keys[1]] - want["subset_mean"]) <= sub_bounds.mean() + host
    assert abs(outs["kid"][keys[2]] - want["subset_std"]) <= sub_bounds.max() + host
    with pytest.raises(ValueError, match="kid=True needs a classifier"):
        model.evaluate(str(tmp_path), None, None, kid=True)
    with pytest.raises(ValueError, match="kid=True needs a classifier"):
        model.evaluate(str(tmp_path), None, None, swd=True, kid=True)
    with pytest.raises(ValueError, match="kid_subset_size must be an integer >= 2"):
        model.evaluate(str(tmp_path), None, clf, kid=True, kid_subset_size=1)
    with pytest.raises(ValueError, match="kid_subsets must be an integer >= 0"):
        model.evaluate(str(tmp_path), None, clf, kid=True, kid_subsets=-1)


def test_gan_synth_main_kid(tmp_path):
    from tests.test_classifier_gpu import _classifier_file
    clf = _classifier_file(tmp_path / "clf.safetensors", seed=10)
    cmd = [sys.executable, os.path.join(ROOT, "gan_synth_main.py"), "--evaluate", "--synthetic", "--kid", "--kid_subsets", "6", "--classifier", clf,
           "--model_dir", str(tmp_path / "model"), "--batch_size", "8", "--num_generate_batches", "3"]
    r = subprocess.run(cmd, cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    line = [s for s in r.stdout.splitlines() if "frechet_inception_distance" in s][-1]
    print(line)
    keys = ("kernel_inception_distance", "kernel_inception_distance_subset_mean", "kernel_inception_distance_subset_std")
    assert all(f"'{key}'" in line for key in keys) and "inception_score" not in line and "precision" not in line
