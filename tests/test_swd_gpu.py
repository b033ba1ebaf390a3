"""GPU: every gs_swd entry element-wise against the float64 restatement (tests/swd_ref.py, where every bound lives with its derivation), then
metrics.sliced_wasserstein_distance_device, GANSynth.evaluate(swd=True) and the driver's --swd.  Every figure is printed before it is asserted.

The kernel tests call the C entries themselves: the inputs sit inside NaN-filled buffers, once 16-byte aligned and once one float off, every
output inside a sentinel-filled buffer, and nothing outside the outputs may change (the sort works in place: its rows sit inside NaN)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import swd_ref as SR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD = 64                                   # elements of sentinel on either side of every buffer
F_SENT = -12345.5
TILE = SR.SORT_TILE
ALIGNED = pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "one float off"])


def _lib():
    from gansynth_amd import _lib as L
    return L, L.load()


def _stream():
    from gansynth_amd import kernels
    return kernels._stream()


def _ws(stage, a, b=0, c=0):
    from gansynth_amd import kernels
    L, lib = _lib()
    need = lib.gs_swd_workspace_bytes(stage, a, b, c)
    assert need > 0
    return kernels._ws(need, torch.device("cuda"))


def _place(a, aligned, dtype=torch.float32):
    """The values of `a` (any shape, flattened) inside a NaN-filled device buffer, the first on 16 bytes or one float (4 bytes) off."""
    per_float = 4 // torch.empty((), dtype=dtype).element_size()
    off = PAD + (0 if aligned else per_float)
    buf = torch.full((off + a.size + PAD,), float("nan"), dtype=dtype, device="cuda")
    view = buf[off:off + a.size]
    view.copy_(torch.from_numpy(np.array(a).reshape(-1)).to(dtype))
    assert (view.data_ptr() % 16 == 0) == aligned
    return buf, view


def _out(count, sentinel, dtype, aligned=True):
    """`count` elements inside a sentinel-filled buffer, the first on 16 bytes or one element off: -> (buffer, view)."""
    off = PAD + (0 if aligned else 1)
    buf = torch.full((off + count + PAD,), sentinel, dtype=dtype, device="cuda")
    return buf, buf[off:off + count]


def _intact(buf, view, sentinel=None):
    """Nothing around `view` inside `buf` was written (sentinel None: the surroundings are NaN)."""
    host = buf.float().cpu().numpy() if buf.dtype == torch.bfloat16 else buf.cpu().numpy()
    off = (view.data_ptr() - buf.data_ptr()) // buf.element_size()
    around = np.concatenate([host[:off], host[off + view.numel():]])
    return bool(np.isnan(around).all() if sentinel is None else (around == sentinel).all())


# ----------------------------------------------------------------------------------------------------------------- pyramid
@functools.lru_cache(maxsize=None)
def _images(n, h, w, bf16):
    rng = np.random.default_rng(n * 1000 + h + w)
    x = (1.5 * rng.standard_normal((n, 2, h, w)) + 0.3).astype(np.float32)
    if bf16:
        x = torch.from_numpy(x).bfloat16().float().numpy()           # exactly representable: the widening is exact
    laps = SR.laplacian(x)
    x.setflags(write=False)
    return x, laps


@ALIGNED
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("n,h,w", [(1, 16, 16), (3, 32, 64), (2, 64, 128)], ids=["1x16x16", "3x32x64", "2x64x128"])
def test_pyramid(n, h, w, dtype, aligned):
    from gansynth_amd import kernels
    L, lib = _lib()
    x, want = _images(n, h, w, dtype == torch.bfloat16)
    count = SR.levels(h, w)
    xbuf, xv = _place(x.transpose(0, 2, 3, 1), aligned, dtype)
    sizes = [n * (h >> l) * (w >> l) * 2 for l in range(count)]
    obuf, out = _out(sum(sizes), F_SENT, torch.float32, aligned)
    ws = _ws(L.SWD_STAGE_PYRAMID, n, h, w)

    def run(dst):
        L.check(lib.gs_swd_pyramid(xv.data_ptr(), L.GS_F32 if dtype == torch.float32 else L.GS_BF16, n, h, w, dst.data_ptr(), ws.data_ptr(), ws.numel(), _stream()),
                "gs_swd_pyramid")
        torch.cuda.synchronize()

    run(out)
    got, at, top = out.cpu().numpy().astype(np.float64), 0, float(np.abs(x).max())
    for l, size in enumerate(sizes):
        level = got[at:at + size].reshape(n, h >> l, w >> l, 2).transpose(0, 3, 1, 2)
        at += size
        err, bound = float(np.abs(level - want[l]).max()), SR.pyramid_bound(l, count, top)
        print(f"{n}x2x{h}x{w} {dtype} level {l}: worst error {err:.3g}, bound {bound:.3g} ({bound / SR.U / top:.1f} u max|x|)")
        assert np.isfinite(level).all() and err <= bound
        if count == 1:
            assert np.array_equal(level, x.astype(np.float64))        # one level: Lap = x, bit for bit
    assert _intact(obuf, out, F_SENT) and _intact(xbuf, xv)
    assert np.array_equal(xv.float().cpu().numpy(), x.transpose(0, 2, 3, 1).reshape(-1))       # the input is as it was
    again = torch.full_like(out, F_SENT)
    run(again)
    assert torch.equal(again, out)                                    # the same bits
    levels = kernels.swd_pyramid(torch.from_numpy(np.array(x)).to("cuda", dtype))              # the Python layer, from a tensor that is not channels-last
    assert len(levels) == count and torch.equal(torch.cat([t.reshape(-1) for t in levels]), out)
    assert [tuple(t.shape) for t in levels] == [(n, h >> l, w >> l, 2) for l in range(count)]


# ----------------------------------------------------------------------------------------------------------------- patches
@ALIGNED
@pytest.mark.parametrize("b,h,w", [(1, 7, 7), (2, 16, 32), (3, 9, 40)], ids=["1x7x7", "2x16x32", "3x9x40"])
def test_patches(b, h, w, aligned):
    L, lib = _lib()
    rng = np.random.default_rng(b + h + w)
    level = rng.standard_normal((b, 2, h, w)).astype(np.float32)
    ys, xs = rng.integers(0, h - 6, (b, 128)), rng.integers(0, w - 6, (b, 128))
    ys[:, 0], xs[:, 0] = 0, 0
    ys[:, 1], xs[:, 1] = h - 7, w - 7                                 # both extreme corners, in every image
    ys[-1, -1], xs[-1, -1] = h - 7, 0
    want = SR.descriptors(level, ys, xs)
    lbuf, lv = _place(level.transpose(0, 2, 3, 1), aligned)
    offset, rows = 5, 5 + b * 128 + 3
    dbuf, desc = _out(rows * 98, F_SENT, torch.float32, aligned)
    ydev, xdev = (torch.from_numpy(c.reshape(-1).astype(np.int32)).cuda() for c in (ys, xs))
    L.check(lib.gs_swd_patches(lv.data_ptr(), b, h, w, ydev.data_ptr(), xdev.data_ptr(), desc.data_ptr(), rows, offset, _stream()), "gs_swd_patches")
    torch.cuda.synchronize()
    got = desc.cpu().numpy().reshape(rows, 98)
    print(f"{b}x{h}x{w}: rows {offset} .. {offset + b * 128} of {rows} equal numpy indexing: {np.array_equal(got[offset:offset + b * 128], want)}")
    assert np.array_equal(got[offset:offset + b * 128], want)
    assert (got[:offset] == F_SENT).all() and (got[offset + b * 128:] == F_SENT).all() and _intact(dbuf, desc, F_SENT) and _intact(lbuf, lv)


def test_patches_python_layer_appends_at_a_row_offset():
    from gansynth_amd import kernels
    rng = np.random.default_rng(4)
    level = rng.standard_normal((2, 2, 16, 32)).astype(np.float32)
    ys, xs = rng.integers(0, 10, (2, 128)), rng.integers(0, 26, (2, 128))
    desc = torch.full((3 * 128, 98), F_SENT, device="cuda")
    dev = torch.from_numpy(np.ascontiguousarray(level.transpose(0, 2, 3, 1))).cuda()
    same = kernels.get().swd_patches(dev, torch.from_numpy(ys.reshape(-1).astype(np.int32)).cuda(), torch.from_numpy(xs.reshape(-1).astype(np.int32)).cuda(), desc, 128)
    assert same is desc and np.array_equal(desc[128:].cpu().numpy(), SR.descriptors(level, ys, xs)) and bool((desc[:128] == F_SENT).all())


# ----------------------------------------------------------------------------------------------------------------- moments
@ALIGNED
@pytest.mark.parametrize("rows", [1, 20, 21, 5000, 30000])            # 2048 values a block: one block, two, many, the cap of 1024
def test_moments(rows, aligned):
    L, lib = _lib()
    rng = np.random.default_rng(rows)
    desc = (rng.standard_normal((rows, 98)) * np.where(np.arange(98) < 49, 0.7, 2.0) + np.where(np.arange(98) < 49, 3.0, -0.25)).astype(np.float32)
    dbuf, dv = _place(desc, aligned)
    obuf, out = _out(8, F_SENT, torch.float64)
    ws = _ws(L.SWD_STAGE_MOMENTS, rows)
    L.check(lib.gs_swd_moments(dv.data_ptr(), rows, out.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "gs_swd_moments")
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    d = desc.astype(np.float64).reshape(rows, 2, 49)
    m = rows * 49
    for c in range(2):
        v = d[:, c].reshape(-1)
        s, ss, mean, std = np.sum(v), np.sum(v * v), np.mean(v), np.std(v)
        bs, bss = SR.moments_bound(m, np.abs(v).sum()), SR.moments_bound(m, ss)
        # mean = sum / m: the sum's bound over m and one rounding; var = sumsq / m - mean^2: both bounds over m, four roundings of values of at most
        # sumsq / m; std = sqrt(var): an error of var over std covers the derivative 1 / (2 std) and the root's rounding
        bmean = bs / m + 2.0 ** -52 * abs(mean)
        bstd = ((bss + 2 * abs(mean) * bs) / m + 4 * 2.0 ** -52 * ss / m) / std
        print(f"rows {rows} channel {c}: sum {abs(got[4 * c] - s):.3g} (bound {bs:.3g}), sumsq {abs(got[4 * c + 1] - ss):.3g} ({bss:.3g}), "
              f"mean {abs(got[4 * c + 2] - mean):.3g} ({bmean:.3g}), std {abs(got[4 * c + 3] - std):.3g} ({bstd:.3g})")
        assert abs(got[4 * c] - s) <= bs and abs(got[4 * c + 1] - ss) <= bss
        assert abs(got[4 * c + 2] - mean) <= bmean and abs(got[4 * c + 3] - std) <= bstd
    assert _intact(obuf, out, F_SENT) and _intact(dbuf, dv)
    again = torch.empty_like(out)
    L.check(lib.gs_swd_moments(dv.data_ptr(), rows, again.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "gs_swd_moments")
    assert torch.equal(again, out)


def test_moments_of_constant_channels_have_standard_deviation_zero():
    from gansynth_amd import kernels, metrics
    got = kernels.get().swd_moments(torch.zeros(256, 98, device="cuda")).cpu().numpy()
    assert (got == 0.0).all()
    with pytest.raises(ValueError, match="standard deviation 0"):
        metrics.sliced_wasserstein_distance_device(torch.zeros(2, 2, 16, 16), torch.ones(2, 2, 16, 16))


# ----------------------------------------------------------------------------------------------------------------- projection
@ALIGNED
@pytest.mark.parametrize("n,ndir", [(1, 512), (127, 512), (128, 33), (129, 512), (300, 1), (300, 512)])
def test_project(n, ndir, aligned):
    L, lib = _lib()
    rng = np.random.default_rng(n + ndir)
    desc = (rng.standard_normal((n, 98)) * 1.3 + 0.4).astype(np.float32)
    dirs = SR.directions(7)[:, :ndir].copy()
    mean, std = np.array([0.4123456789, 0.38]), np.array([1.29, 1.3111111])
    moments = torch.tensor([0.0, 0.0, mean[0], std[0], 0.0, 0.0, mean[1], std[1]], dtype=torch.float64, device="cuda")
    a = SR.normalise(desc, mean.astype(np.float32), std.astype(np.float32))     # exact quotients of the fp32 mean and std the kernel uses
    want, bound = a @ dirs.astype(np.float64), SR.project_bound(np.abs(a) @ np.abs(dirs.astype(np.float64)))
    dbuf, dv = _place(desc, aligned)
    rbuf, rv = _place(dirs, aligned)
    obuf, out = _out(ndir * n, F_SENT, torch.float32, aligned)
    L.check(lib.gs_swd_project(dv.data_ptr(), n, moments.data_ptr(), rv.data_ptr(), ndir, out.data_ptr(), _stream()), "gs_swd_project")
    torch.cuda.synchronize()
    got = out.cpu().numpy().astype(np.float64).reshape(ndir, n).T
    err = np.abs(got - want)
    print(f"n {n} ndir {ndir}: worst error {err.max():.3g}, {float((err / bound).max()):.3g} of its bound (101 u sum |a| |d|)")
    assert np.isfinite(got).all() and (err <= bound).all()
    assert _intact(obuf, out, F_SENT) and _intact(dbuf, dv) and _intact(rbuf, rv)
    again = torch.full_like(out, F_SENT)
    L.check(lib.gs_swd_project(dv.data_ptr(), n, moments.data_ptr(), rv.data_ptr(), ndir, again.data_ptr(), _stream()), "gs_swd_project")
    assert torch.equal(again, out)


# ----------------------------------------------------------------------------------------------------------------- sort
SORT_N = [1, 2, 63, 64, 65, 1000, 1024, 1025, 4097, TILE - 1, TILE, TILE + 1, 3 * TILE + 1, 4 * TILE + 1]      # the last one: five tiles, three merge passes


def _sort_inputs(rows, n, seed):
    rng = np.random.default_rng(seed)
    gauss = rng.standard_normal((rows, n)).astype(np.float32)
    zeros = rng.choice(np.array([0.0, -0.0, -1.5, -3.0e-39, 2.0], dtype=np.float32), (rows, n))       # both zeros, negatives, a denormal
    return {"Gaussians": gauss, "sorted": np.sort(gauss, axis=1), "reversed": np.sort(gauss, axis=1)[:, ::-1].copy(), "all equal": np.full((rows, n), 2.5, dtype=np.float32),
            "8-value alphabet": rng.choice(gauss[0, :8] if n >= 8 else np.arange(8, dtype=np.float32), (rows, n)).astype(np.float32), "zeros of both signs": zeros}


@ALIGNED
@pytest.mark.parametrize("rows", [1, 3, 128])
@pytest.mark.parametrize("n", SORT_N)
def test_sort(n, rows, aligned):
    L, lib = _lib()
    ws = _ws(L.SWD_STAGE_SORT, rows, n)
    passes = max(0, int(np.ceil(np.log2(-(-n // TILE)))))
    for name, data in _sort_inputs(rows, n, 31 * n + rows).items():
        buf, view = _place(data, aligned)
        L.check(lib.gs_swd_sort(view.data_ptr(), rows, n, ws.data_ptr(), ws.numel(), _stream()), "gs_swd_sort")
        torch.cuda.synchronize()
        got = view.cpu().numpy().reshape(rows, n)
        same = np.array_equal(got, np.sort(data, axis=1))
        print(f"rows {rows} n {n} ({passes} merge passes) {name}: equal to np.sort {same}")
        assert same
        assert np.array_equal(np.sort(got.view(np.uint32), axis=1), np.sort(data.view(np.uint32), axis=1))     # a permutation, bit for bit (no zero changed its sign)
        assert _intact(buf, view)                                     # the NaN around the rows is where it was, and none reached a row
    assert passes >= 3 or n != SORT_N[-1]


def test_sort_python_layer():
    from gansynth_amd import kernels
    data = torch.randn(5, 9000, device="cuda")
    want = np.sort(data.cpu().numpy(), axis=1)
    assert kernels.swd_sort(data) is data and np.array_equal(data.cpu().numpy(), want)
    with pytest.raises(ValueError, match="data must be on the HIP device"):
        kernels.swd_sort(torch.zeros(2, 10))


# ----------------------------------------------------------------------------------------------------------------- L1
@ALIGNED
@pytest.mark.parametrize("rows,n", [(1, 1), (1, 2048), (1, 2049), (3, 1000), (128, 4097), (3, 700001)])     # one block, two, many, the cap of 1024
def test_l1(rows, n, aligned):
    L, lib = _lib()
    rng = np.random.default_rng(rows + n)
    a, b = rng.standard_normal((rows, n)).astype(np.float32), (rng.standard_normal((rows, n)) * 1.2 + 0.1).astype(np.float32)
    abuf, av = _place(a, aligned)
    bbuf, bv = _place(b, aligned)
    obuf, out = _out(1, F_SENT, torch.float64)
    ws = _ws(L.SWD_STAGE_L1, rows, n)

    def run(p, q):
        L.check(lib.gs_swd_l1(p.data_ptr(), q.data_ptr(), rows, n, out.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "gs_swd_l1")
        torch.cuda.synchronize()
        return float(out.item())

    got, want = run(av, bv), float(np.abs(a.astype(np.float64) - b).sum())
    print(f"rows {rows} n {n}: {got!r} against {want!r}: error {abs(got - want):.3g}, bound {SR.moments_bound(rows * n, want):.3g}")
    assert abs(got - want) <= SR.moments_bound(rows * n, want)        # every difference is exact in double: the sum's roundings only
    assert run(av, bv) == got and run(bv, av) == got
    assert run(av, av) == 0.0
    assert _intact(obuf, out, F_SENT) and _intact(abuf, av) and _intact(bbuf, bv)


# ----------------------------------------------------------------------------------------------------------------- the whole metric
@pytest.mark.parametrize("n,h,w", [(4, 32, 64), (3, 64, 128)], ids=["4x2x32x64", "3x2x64x128"])
def test_metric_against_the_restatement(n, h, w):
    from gansynth_amd import metrics
    real, fake = SR.prototype(n, h, w)
    ref = SR.swd(real, fake)
    details = {}
    got = metrics.sliced_wasserstein_distance_device(real, fake, details=details)
    for l, (mine, want) in enumerate(zip(details["levels"], ref["levels"])):
        print(f"{n}x2x{h}x{w} level {ref['sizes'][l]}: {mine!r} against {want!r}: error {abs(mine - want):.3g}, bound {SR.metric_bound(ref, l):.3g}")
    assert details["sizes"] == ref["sizes"] and details["n"] == n and len(details["levels"]) == SR.levels(h, w)
    assert all(abs(mine - want) <= SR.metric_bound(ref, l) for l, (mine, want) in enumerate(zip(details["levels"], ref["levels"])))
    assert got == float(np.mean(details["levels"])) and abs(got - ref["mean"]) <= max(SR.metric_bound(ref, l) for l in range(len(ref["levels"])))
    again = {}
    assert metrics.sliced_wasserstein_distance_device(torch.from_numpy(np.array(real)).cuda(), torch.from_numpy(np.array(fake)), details=again) == got
    assert again["levels"] == details["levels"]                       # a second call: the same bits


def test_identical_sets_with_identical_corners_give_zero():
    from gansynth_amd import swd
    real, _ = SR.prototype(4, 32, 64)
    acc = swd.SlicedWasserstein((32, 64), seed=9)
    acc.rngs[1] = np.random.Generator(np.random.PCG64(9))             # the fake set draws the real set's corners
    x = torch.from_numpy(np.array(real)).cuda()
    acc.add(x[:3], x[:3].clone())
    acc.add(x[3:], x[3:].clone())
    out = acc.result()
    print(out)
    assert out["levels"] == [0.0, 0.0] and out["mean"] == 0.0 and out["n"] == 4
    other = swd.SlicedWasserstein((32, 64), seed=9)                   # its own corners: the same images no longer give 0
    other.add(x, x.clone())
    assert min(other.result()["levels"]) > 0.0


# ----------------------------------------------------------------------------------------------------------------- evaluate and the driver
def test_evaluate_with_swd(tmp_path, gpu_store):
    from gansynth_amd import checkpoint, metrics, swd
    from tests.test_classifier_gpu import _classifier_file, _gan
    clf = _classifier_file(tmp_path / "clf.safetensors")
    seen, original = [], swd.SlicedWasserstein.add

    def recording(self, real, fake):
        seen.append((real.clone(), fake.clone()))
        return original(self, real, fake)

    outs = {}
    for mode in ("plain", "swd", "alone"):
        model = _gan(8, 3)
        model._ensure_built(torch.randn(8, 256, device="cuda"), torch.eye(61, device="cuda")[:8])
        if mode == "plain":
            checkpoint.save(model, str(tmp_path))
        swd.SlicedWasserstein.add = recording if mode == "swd" else original
        try:
            extra = {}
            kw = {} if mode == "plain" else dict(swd=True, swd_seed=4, features_out=extra)
            outs[mode] = model.evaluate(str(tmp_path), None, None if mode == "alone" else clf, "images:0", ["features:0", "logits:0"], **kw)
        finally:
            swd.SlicedWasserstein.add = original
        print(mode, outs[mode])
    keys = {"sliced_wasserstein_distance", "sliced_wasserstein_distance_levels"}
    assert set(outs["plain"]) == {"frechet_inception_distance"} and set(outs["swd"]) == set(outs["plain"]) | keys and set(outs["alone"]) == keys
    assert outs["swd"]["frechet_inception_distance"] == outs["plain"]["frechet_inception_distance"]
    assert all(outs["alone"][key] == outs["swd"][key] for key in keys)                     # classifier=None: the same figures, and only them
    assert extra["swd_sizes"] == ["128x1024", "64x512", "32x256", "16x128"] and len(outs["swd"]["sliced_wasserstein_distance_levels"]) == 4
    assert len(seen) == 3 and seen[0][0].shape == (8, 2, 128, 1024)
    details = {}
    whole = metrics.sliced_wasserstein_distance_device(torch.cat([r for r, _ in seen]), torch.cat([f for _, f in seen]), seed=4, details=details, batch_size=8)
    assert whole == outs["swd"]["sliced_wasserstein_distance"] and details["levels"] == outs["swd"]["sliced_wasserstein_distance_levels"]
    with pytest.raises(ValueError, match="classifier=None needs swd=True"):
        model.evaluate(str(tmp_path), None, None)


def test_gan_synth_main_swd(tmp_path):
    cmd = [sys.executable, os.path.join(ROOT, "gan_synth_main.py"), "--evaluate", "--swd", "--synthetic", "--classifier", "none",
           "--model_dir", str(tmp_path / "model"), "--batch_size", "8", "--num_generate_batches", "2"]
    r = subprocess.run(cmd, cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    line = [s for s in r.stdout.splitlines() if "sliced_wasserstein_distance" in s][-1]
    print(line)
    assert "'sliced_wasserstein_distance'" in line and "'sliced_wasserstein_distance_levels'" in line and "frechet" not in line
