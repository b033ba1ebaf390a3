"""CPU: the rules of gansynth_amd/swd.py against their float64 restatement (tests/swd_ref.py) -- the pyramid reconstructs its input, the corner
and direction streams are pinned, the level counts --, every refusal of the gs_swd entries and of the Python layer without a launch, the
workspace arithmetic, and GANSynth.evaluate(swd=True) on a reduced network under a CPU backend that computes the kernel layer's SWD methods
in numpy (a subclass of tests/cpu_kernels.CpuEmuKernels, below).  Every figure is printed before it is asserted."""
import numpy as np
import pytest
import torch

from tests import swd_ref as SR
from tests.cpu_kernels import CpuEmuKernels


# ------------------------------------------------------------------------------------------------------------- the rules
def test_the_float64_pyramid_reconstructs_its_input():
    rng = np.random.default_rng(0)
    exact = rng.integers(-8, 9, (4, 2, 32, 64)).astype(np.float64)    # small integers and dyadic weights: every operation is exact
    err = np.abs(SR.reconstruct(SR.laplacian(exact)) - exact).max()
    print(f"integers: reconstruction error {err!r}")
    assert err == 0.0
    x = rng.standard_normal((4, 2, 32, 64))
    laps = SR.laplacian(x)
    err = np.abs(SR.reconstruct(laps) - x).max()
    print(f"Gaussians: reconstruction error {err!r} (two roundings a level: bound {4 * 2.0 ** -53 * np.abs(x).max() * 2!r})")
    assert [lap.shape[-2:] for lap in laps] == [(32, 64), (16, 32)]
    assert err <= 8 * 2.0 ** -53 * np.abs(x).max()             # (g - up) + up: two roundings of values of at most 2 max|x|, per level
    const = np.full((1, 2, 32, 64), 3.0)
    assert np.abs(SR.laplacian(const)[0]).max() == 0.0 and (SR.down(const) == 3.0).all()     # the weights add up to 1 in every phase, border included


def test_the_border_is_mirrored_without_the_edge_sample():
    row = np.arange(16.0).reshape(1, 1, 1, 16) * np.ones((1, 1, 16, 1))
    got = SR.down(row)[0, 0, 0]
    # column 0: (1 * x[2] + 4 * x[1] + 6 * x[0] + 4 * x[1] + 1 * x[2]) / 16 = 12 / 16; column 2 (inside): x[4] = 4
    print(got[:3].tolist())
    assert got[0] == 0.75 and got[1] == 2.0 and got[2] == 4.0
    up = SR.up(np.arange(8.0).reshape(1, 1, 1, 8) * np.ones((1, 1, 8, 1)))[0, 0, 0]
    # stuffed row 0 _ 1 _ 2 ...: out[0] = (6 * 0 + 1 * 1 + 1 * 1) / 8 (the mirror of index -2 is 2: coarse 1); out[1] = (4 * 0 + 4 * 1) / 8;
    # out[15] = (4 * 7 + 4 * 7) / 8: index 16 mirrors to 14, coarse 7
    assert up[0] == 0.25 and up[1] == 0.5 and up[2] == 1.0 and up[15] == 7.0 and up[14] == (6 * 7 + 6 + 7) / 8


def test_the_streams_are_pinned():
    from gansynth_amd import swd
    picks = SR.corners(0, [3, 1], 32, 64)
    assert picks[0][0].shape == (4, 128) and picks[0][0].max() <= 25 and picks[0][1].max() <= 57 and picks[1][0].max() <= 9 and picks[1][1].max() <= 25
    assert picks[0][0][0, :4].tolist() == [22, 16, 13, 7] and picks[0][1][0, :4].tolist() == [43, 30, 17, 5]
    assert picks[1][0][3, :4].tolist() == [4, 1, 5, 4] and picks[1][1][3, -3:].tolist() == [1, 21, 21]
    assert SR.corners(1, [4], 32, 64)[0][0][0, :4].tolist() == [12, 13, 19, 24]           # the fake set of seed 0
    rng = np.random.Generator(np.random.PCG64(0))
    first = swd.draw_corners(rng, 3, 32, 64, 2)
    second = swd.draw_corners(rng, 1, 32, 64, 2)
    for l in range(2):
        for axis in range(2):
            assert np.array_equal(np.concatenate([first[l][axis], second[l][axis]]).reshape(4, 128), picks[l][axis])
            assert first[l][axis].dtype == np.int32
    d = SR.directions(0)
    assert d.shape == (98, 512) and d.dtype == np.float32
    assert [float(v) for v in d[0, :3]] == [0.018622292205691338, -0.053254347294569016, -0.041271425783634186]
    assert float(d[97, 511]) == -0.17493130266666412 and float(d[5, 128]) == 0.06481903046369553
    assert np.abs((d.astype(np.float64) ** 2).sum(axis=0) - 1.0).max() <= 98 * SR.U
    assert np.array_equal(swd.directions(0), d) and not np.array_equal(swd.directions(1), d)


def test_level_counts():
    from gansynth_amd import _lib, kernels
    lib = _lib.load()
    cases = [((16, 16), 1), ((32, 64), 2), ((128, 1024), 4), ((64, 128), 3), ((24, 24), 1), ((34, 64), 2), ((100, 100), 3),
             ((15, 16), 0), ((16, 15), 0), ((8, 1024), 0), ((70, 70), 0), ((33, 64), 0), ((64, 66), 0), ((16, 16385), 0), ((0, 0), 0), ((-32, 64), 0)]
    for (h, w), want in cases:
        got = (lib.gs_swd_levels(h, w), kernels.swd_levels(h, w), SR.levels(h, w))
        print(f"{h} x {w}: library, package, restatement {got}, by hand {want}")
        assert got == (want, want, want)
    assert (_lib.SWD_DESC, _lib.SWD_PATCHES, _lib.SWD_SORT_TILE, _lib.SWD_MAX_N, _lib.SWD_MAX_ROWS, _lib.SWD_MAX_SIDE, _lib.SWD_MAX_BATCH) == \
        (SR.DESC, SR.PATCHES, SR.SORT_TILE, SR.MAX_N, SR.MAX_ROWS, SR.MAX_SIDE, SR.MAX_BATCH)
    assert _lib.SWD_MAX_N >= 2 ** 21


def test_the_bounds_by_hand():
    u = SR.U
    assert abs(SR.gaussian_error(1, 1.0) / u - 8.0) < 1e-4 and SR.gaussian_error(0, 5.0) == 0.0
    assert SR.pyramid_bound(0, 1, 3.0) == 0.0                                              # one level: Lap = x
    assert abs(SR.pyramid_bound(0, 2, 1.0) / u - 14.0) < 1e-4                              # 8 (down) + 4 (up) + 2 (the subtraction of values below 2)
    assert abs(SR.pyramid_bound(1, 2, 1.0) / u - 8.0) < 1e-4
    assert SR.project_bound(2.0) == 101 * u * 2.0 and SR.moments_bound(1000, 3.0) == 3000 * 2.0 ** -52


# ------------------------------------------------------------------------------------------------------------- the C entries
def test_workspace_arithmetic():
    from gansynth_amd import _lib
    lib = _lib.load()
    by_hand = [((0, 8, 128, 1024), 4 * 8 * 2 * (64 * 512 + 32 * 256 + 16 * 128) + 16), ((0, 1, 16, 16), 16), ((0, 3, 32, 64), 4 * 3 * 2 * 16 * 32 + 16),
               ((1, 512, 0, 0), 32 * 25),                       # 512 * 98 values: 25 blocks of four doubles
               ((1, 2 ** 20, 0, 0), 32 * 1024), ((2, 512, 4096, 0), 16), ((2, 512, 4097, 0), 512 * 4097 * 4), ((2, 512, 2 ** 20, 0), 2 ** 31),
               ((3, 512, 2 ** 20, 0), 8 * 1024), ((3, 1, 1, 0), 16)]
    for args, want in by_hand:
        got = lib.gs_swd_workspace_bytes(*args)
        print(f"{args}: library {got}, restatement {SR.workspace_bytes(*args)}, by hand {want}")
        assert got == SR.workspace_bytes(*args) == want
    refused = [(0, 0, 32, 64), (0, 1, 33, 64), (0, 1, 8, 8), (0, 2 ** 16 + 1, 32, 64), (1, 0, 0, 0), (1, 2 ** 21 + 1, 0, 0), (2, 0, 5, 0), (2, 5, 0, 0),
               (2, 1, 2 ** 21 + 1, 0), (2, 65536, 5, 0), (3, 1, 2 ** 21 + 1, 0), (3, 0, 1, 0), (4, 1, 1, 1), (-1, 1, 1, 1)]
    for args in refused:
        assert lib.gs_swd_workspace_bytes(*args) == 0 == SR.workspace_bytes(*args), args


def test_abi_refusals():
    """Dummy pointers: the argument checks come first, nothing is dereferenced or launched; every message names its entry and its argument."""
    from gansynth_amd import _lib
    lib = _lib.load()
    P, BIG = 0x10000, 1 << 40
    g = dict(x=P, dtype=_lib.GS_F32, b=3, h=32, w=64, out=P, ws=P, ws_bytes=BIG, ys=P, xs=P, desc_rows=1000, row_offset=0, rows=4, n=5000, moments=P, dirs=P, ndir=512,
             other=P)

    def pyramid(a):
        return lib.gs_swd_pyramid(a["x"], a["dtype"], a["b"], a["h"], a["w"], a["out"], a["ws"], a["ws_bytes"], None)

    def patches(a):
        return lib.gs_swd_patches(a["x"], a["b"], a["h"], a["w"], a["ys"], a["xs"], a["out"], a["desc_rows"], a["row_offset"], None)

    def moments(a):
        return lib.gs_swd_moments(a["x"], a["n"], a["out"], a["ws"], a["ws_bytes"], None)

    def project(a):
        return lib.gs_swd_project(a["x"], a["n"], a["moments"], a["dirs"], a["ndir"], a["out"], None)

    def sort(a):
        return lib.gs_swd_sort(a["x"], a["rows"], a["n"], a["ws"], a["ws_bytes"], None)

    def l1(a):
        return lib.gs_swd_l1(a["x"], a["other"], a["rows"], a["n"], a["out"], a["ws"], a["ws_bytes"], None)

    null = [(dict(x=None), b"null pointer"), (dict(out=None), b"null pointer"), (dict(x=P + 2), b"misaligned")]
    ws = lambda stage, *args: [(dict(ws=None), b"workspace"), (dict(ws=P + 8), b"workspace"), (dict(ws_bytes=0), b"workspace"),   # noqa: E731
                               (dict(ws_bytes=int(lib.gs_swd_workspace_bytes(stage, *args)) - 1), b"workspace")]
    too_long = [(dict(n=0), b"must be in"), (dict(n=2 ** 21 + 1), b"must be in"), (dict(n=-4), b"must be in")]
    rows = [(dict(rows=0), b"rows must be in"), (dict(rows=65536), b"rows must be in")]
    table = [
        (pyramid, b"swd_pyramid", null + ws(0, 3, 32, 64) + [(dict(h=33), b"no level"), (dict(w=70, h=70), b"no level"), (dict(h=8), b"no level"), (dict(w=15), b"no level"),
                                                              (dict(h=2 ** 15), b"no level"), (dict(b=0), b"b must be in"), (dict(b=2 ** 16 + 1), b"b must be in"),
                                                              (dict(dtype=2), b"bad dtype"), (dict(dtype=-1), b"bad dtype")]),
        (patches, b"swd_patches", null + [(dict(ys=None), b"null pointer"), (dict(xs=None), b"null pointer"), (dict(ys=P + 1), b"misaligned"), (dict(h=6), b"7 x 7"),
                                          (dict(w=0), b"7 x 7"), (dict(b=0), b"b must be in"), (dict(row_offset=-1), b"do not lie inside"),
                                          (dict(row_offset=1000 - 3 * 128 + 1), b"do not lie inside"), (dict(desc_rows=383), b"do not lie inside"),
                                          (dict(desc_rows=2 ** 21 + 1), b"desc_rows must be in"), (dict(desc_rows=0), b"desc_rows must be in")]),
        (moments, b"swd_moments", null + ws(1, 5000, 0, 0) + too_long + [(dict(out=P + 4), b"misaligned")]),
        (project, b"swd_project", null + too_long + [(dict(moments=None), b"null pointer"), (dict(dirs=None), b"null pointer"), (dict(moments=P + 4), b"misaligned"),
                                                     (dict(ndir=0), b"ndir must be in"), (dict(ndir=65536), b"ndir must be in")]),
        (sort, b"swd_sort", [(dict(x=None), b"null pointer"), (dict(x=P + 2), b"misaligned")] + ws(2, 4, 5000, 0) + too_long + rows),
        (l1, b"swd_l1", null + ws(3, 4, 5000, 0) + too_long + rows + [(dict(other=None), b"null pointer"), (dict(out=P + 4), b"misaligned")]),
    ]
    count = 0
    for entry, name, cases in table:
        for change, message in cases:
            assert entry(dict(g, **change)) == -1, (name, change)
            err = lib.gs_last_error()
            print(name.decode(), change, "->", err.decode())
            assert message in err and name in err, (name, change, err)
            count += 1
    assert count == 77


# ------------------------------------------------------------------------------------------------------------- the Python layer
def _raises(fn, *args, match, **kw):
    with pytest.raises(ValueError, match=match):
        fn(*args, **kw)


def test_python_layer_refusals_need_no_device():
    from gansynth_amd import kernels, metrics, swd
    ok = torch.zeros(3, 2, 32, 64)
    assert kernels.swd_pyramid_shapes(ok) == (3, 32, 64, 2) and kernels.swd_pyramid_shapes(ok.bfloat16()) == (3, 32, 64, 2)
    for bad in (np.zeros((3, 2, 32, 64), dtype=np.float32), torch.zeros(2, 32, 64), torch.zeros(3, 2, 32, 64, dtype=torch.float64), torch.zeros(0, 2, 32, 64)):
        _raises(kernels.swd_pyramid_shapes, bad, match="swd_pyramid: images must be")
    _raises(kernels.swd_pyramid_shapes, torch.zeros(3, 3, 32, 64), match="2 channels")
    for bad in (torch.zeros(1, 2, 33, 64), torch.zeros(1, 2, 8, 64), torch.zeros(1, 2, 70, 70)):
        _raises(kernels.swd_pyramid_shapes, bad, match="have no level")
        _raises(kernels.swd_pyramid, bad, match="have no level")
        _raises(swd.SlicedWasserstein, bad.shape, match="have no level")
    level, ys, desc = torch.zeros(2, 16, 32, 2), torch.zeros(256, dtype=torch.int32), torch.zeros(600, 98)
    assert kernels.swd_patches_shapes(level, ys, ys, desc, 344) == (2, 16, 32)
    _raises(kernels.swd_patches_shapes, level, ys, ys, desc, 345, match="do not lie inside")
    _raises(kernels.swd_patches_shapes, level, ys[:255], ys, desc, 0, match="ys must be")
    _raises(kernels.swd_patches_shapes, level, ys, ys.long(), desc, 0, match="xs must be")
    _raises(kernels.swd_patches_shapes, level, ys, ys, torch.zeros(600, 97), 0, match="desc must be")
    _raises(kernels.swd_patches_shapes, torch.zeros(2, 2, 16, 32), ys, ys, desc, 0, match="level must be")
    _raises(kernels.swd_desc_shapes, "swd_moments", torch.zeros(5, 99), match="swd_moments: desc must be")
    moments, dirs = torch.zeros(8, dtype=torch.float64), torch.zeros(98, 512)
    assert kernels.swd_project_shapes(desc, moments, dirs) == (600, 512)
    _raises(kernels.swd_project_shapes, desc, moments.float(), dirs, match="moments must be")
    _raises(kernels.swd_project_shapes, desc, moments, torch.zeros(512, 98), match="dirs must be")
    assert kernels.swd_rows_shapes("swd_sort", "data", torch.zeros(3, 1000)) == (3, 1000)
    _raises(kernels.swd_sort, torch.zeros(3, 2000)[:, ::2], match="swd_sort: data must be contiguous")
    _raises(kernels.swd_sort, torch.zeros(1, 2 ** 21 + 1), match="at most 65535 rows of at most 2097152")
    _raises(kernels.swd_sort, torch.zeros(10), match="swd_sort: data must be")
    _raises(kernels.swd_l1, torch.zeros(3, 10), torch.zeros(3, 11), match="differ in shape")
    _raises(metrics.sliced_wasserstein_distance_device, ok, torch.zeros(4, 2, 32, 64), match="differ in shape")
    _raises(metrics.sliced_wasserstein_distance_device, ok[0], ok[0], match="must be a non-empty")
    acc = swd.SlicedWasserstein((32, 64))
    assert acc.levels == 2 and acc.sizes() == ["32x64", "16x32"]
    _raises(acc.add, ok, torch.zeros(2, 2, 32, 64), match="must both be")
    _raises(acc.add, torch.zeros(3, 2, 64, 64), torch.zeros(3, 2, 64, 64), match="must both be")
    _raises(acc.result, match="no batch was added")


# ------------------------------------------------------------------------------------------------------------- evaluate on a CPU backend
class SwdCpuKernels(CpuEmuKernels):
    """The kernel layer's SWD methods in fp32 numpy (the restatement's functions on fp32 arrays): what swd.py and GANSynth.evaluate call."""

    def swd_pyramid(self, images):
        return [torch.from_numpy(np.ascontiguousarray(lap.transpose(0, 2, 3, 1)).astype(np.float32)) for lap in SR.laplacian(images.float().numpy())]

    def swd_patches(self, level, ys, xs, desc, row_offset=0):
        b = level.shape[0]
        rows = SR.descriptors(level.numpy().transpose(0, 3, 1, 2), ys.numpy().reshape(b, -1), xs.numpy().reshape(b, -1))
        desc[row_offset:row_offset + len(rows)] = torch.from_numpy(rows)
        return desc

    def swd_moments(self, desc):
        mean, std = SR.channel_moments(desc.numpy())
        d = desc.numpy().astype(np.float64).reshape(-1, 2, 49)
        return torch.tensor([d[:, 0].sum(), (d[:, 0] ** 2).sum(), mean[0], std[0], d[:, 1].sum(), (d[:, 1] ** 2).sum(), mean[1], std[1]], dtype=torch.float64)

    def swd_project(self, desc, moments, dirs):
        m = moments.numpy()
        a = SR.normalise(desc.numpy(), m[[2, 6]].astype(np.float32), m[[3, 7]].astype(np.float32)).astype(np.float32)
        return torch.from_numpy(np.ascontiguousarray((a @ dirs.numpy()).T))

    def swd_sort(self, data):
        data.copy_(torch.from_numpy(np.sort(data.numpy(), axis=1)))
        return data

    def swd_l1(self, a, b):
        return torch.tensor([np.abs(a.numpy().astype(np.float64) - b.numpy()).sum()], dtype=torch.float64)


@pytest.fixture
def swd_backend():
    from gansynth_amd import kernels, variables
    old_k, old_s = kernels._K, variables._default
    kernels.set_backend(SwdCpuKernels())
    variables.set_default_store(variables.VariableStore(device="cpu"))
    yield
    kernels._K, variables._default = old_k, old_s


def _model(batches=3, batch=4):
    """A reduced GAN that ends at 16 x 128 (one SWD level): real images straight from the input function."""
    from gansynth_amd import variables
    from gansynth_amd.models import GANSynth
    from gansynth_amd.networks import PGGAN
    from gansynth_amd.utils import Dict
    from oracle import torch_ref as R
    variables.set_default_store(variables.VariableStore(device="cpu", seed=0))
    pg = PGGAN(min_resolution=[2, 16], max_resolution=[16, 128], min_channels=8, max_channels=16, growing_level=1.0)
    g = torch.Generator().manual_seed(5)
    data = [(torch.randn(batch, 16, generator=g), torch.nn.functional.one_hot(torch.randint(0, 5, (batch,), generator=g), 5).float(),
             torch.from_numpy(SR.smooth(torch.randn(batch, 2, 16, 128, generator=g).numpy().astype(np.float64)).astype(np.float32))) for _ in range(batches)]
    cur = [0, 0]

    def real_input_fn():
        if cur[0] >= batches:
            raise StopIteration
        cur[0] += 1
        return data[cur[0] - 1][2], data[cur[0] - 1][1]

    def fake_input_fn():
        cur[1] += 1
        return data[cur[1] - 1][0]

    return GANSynth(pg.generator, pg.discriminator, real_input_fn, fake_input_fn, None, Dict(R.DEFAULT_HYPER)), data


def test_metric_on_the_cpu_backend_matches_the_restatement(swd_backend):
    """swd.py's own host rules (the streams, the batches, the buffers that grow, the final stages) against the restatement, the kernels replaced
    by fp32 numpy: fp32 against float64 differs by rounding only."""
    from gansynth_amd import metrics
    real, fake = SR.prototype(4, 32, 64)
    for batch_size in (None, 3, 1):
        ref = SR.swd(real, fake, seed=2, batch_size=batch_size)
        details = {}
        got = metrics.sliced_wasserstein_distance_device(real, fake, seed=2, details=details, batch_size=batch_size)
        err = [abs(a - b) for a, b in zip(details["levels"], ref["levels"])]
        print(f"batch_size {batch_size}: {details['levels']} against {ref['levels']}: errors {err}, bounds {[SR.metric_bound(ref, l) for l in range(2)]}")
        assert details["sizes"] == ["32x64", "16x32"] and details["n"] == 4 and got == float(np.mean(details["levels"]))
        assert all(e <= SR.metric_bound(ref, l) for l, e in enumerate(err))
    assert SR.swd(real, fake, seed=2, batch_size=3)["levels"] != SR.swd(real, fake, seed=2)["levels"]      # the corner stream follows the batches
    with pytest.raises(ValueError, match="standard deviation 0"):
        metrics.sliced_wasserstein_distance_device(np.zeros((2, 2, 16, 16), dtype=np.float32), np.ones((2, 2, 16, 16), dtype=np.float32))


def test_evaluate_with_swd_and_without_a_classifier(swd_backend):
    from gansynth_amd import metrics, swd
    model, data = _model()
    seen = []
    original = swd.SlicedWasserstein.add

    def recording(self, real, fake):
        seen.append((real.clone(), fake.clone()))
        return original(self, real, fake)

    swd.SlicedWasserstein.add = recording
    try:
        extra = {}
        out = model.evaluate(None, None, None, swd=True, swd_seed=3, features_out=extra)
    finally:
        swd.SlicedWasserstein.add = original
    print(out, extra)
    assert set(out) == {"sliced_wasserstein_distance", "sliced_wasserstein_distance_levels"} and extra == {"swd_sizes": ["16x128"]}
    assert len(out["sliced_wasserstein_distance_levels"]) == 1 and out["sliced_wasserstein_distance"] == out["sliced_wasserstein_distance_levels"][0] > 0
    assert len(seen) == 3 and all(torch.equal(r, d[2]) for (r, _), d in zip(seen, data))
    details = {}
    whole = metrics.sliced_wasserstein_distance_device(torch.cat([r for r, _ in seen]), torch.cat([f for _, f in seen]), seed=3, details=details, batch_size=4)
    assert whole == out["sliced_wasserstein_distance"] and details["levels"] == out["sliced_wasserstein_distance_levels"]
    with pytest.raises(ValueError, match="classifier=None needs swd=True"):
        _model()[0].evaluate(None, None, None)


class _StubResNet(object):
    """Stands in for the pitch classifier on the CPU (the ResNet's kernels have no CPU emulation): fixed random features of the images."""

    def __new__(cls):
        from gansynth_amd import networks

        class Stub(networks.ResNet):
            def __init__(self):
                self.w = torch.randn(2 * 16 * 128, 24, generator=torch.Generator().manual_seed(1))

            def __call__(self, inputs, name="resnet", reuse=None):
                f = inputs.float().reshape(inputs.shape[0], -1) @ self.w
                return f[:, :16], f[:, 16:21]
        return Stub()


def test_evaluate_without_swd_returns_the_keys_it_returned(swd_backend):
    plain = _model()[0].evaluate(None, None, _StubResNet())
    print(plain)
    assert set(plain) == {"frechet_inception_distance"}
    explicit = _model()[0].evaluate(None, None, _StubResNet(), swd=False)
    assert explicit == plain
    both = _model()[0].evaluate(None, None, _StubResNet(), swd=True)
    assert set(both) == {"frechet_inception_distance", "sliced_wasserstein_distance", "sliced_wasserstein_distance_levels"}
    assert both["frechet_inception_distance"] == plain["frechet_inception_distance"]
    assert both["sliced_wasserstein_distance"] == _model()[0].evaluate(None, None, None, swd=True)["sliced_wasserstein_distance"]
