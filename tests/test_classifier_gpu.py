"""GPU: the pitch classifier's kernels (gansynth_amd/csrc/classifier.hip and the 3x3 convs at 512 channels) against the float64
oracle of tests/resnet_ref.py, a full-size forward, determinism, and GANSynth.evaluate / gan_synth_main.py --evaluate end to end.
Tolerances: 1e-3 of the reference's largest magnitude in fp32; the max pool bit-exact."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import resnet_ref as RR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CL = torch.channels_last


def _K():
    from gansynth_amd import kernels
    return kernels.get()


def _dev(t, dtype=torch.float32):
    return torch.as_tensor(t).to("cuda", dtype).contiguous(memory_format=CL)


def _rel(got, ref):
    got = torch.as_tensor(got).detach().double().cpu()
    ref = torch.as_tensor(ref).double()
    return float((got - ref).abs().max() / ref.abs().max())


def _ws_weight(w):
    """fp32 device copy of the oracle's standardised weight (the conv kernels take standardised weights)."""
    return RR.weight_standardization(w).float().cuda()


def test_weight_standardization():
    from gansynth_amd import ops
    g = torch.Generator().manual_seed(0)
    for shape in [(7, 7, 2, 64), (3, 3, 512, 512), (1, 1, 256, 512)]:
        w = torch.randn(shape, generator=g) * 0.05 + torch.randn(shape[-1], generator=g) * 0.3   # per-channel offsets
        got = ops.weight_standardization(w.cuda())
        assert _rel(got, RR.weight_standardization(w)) < 1e-5, shape


def test_stem_and_pool_at_full_size():
    """128 x 1024 pins the 2 / 3 SAME padding of the 7x7 / 2 stem; the fused pool equals the max pool of the stem bit for bit."""
    K = _K()
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 2, 128, 1024, generator=g)
    w = torch.randn(7, 7, 2, 64, generator=g) * 0.2
    b = torch.randn(64, generator=g) * 0.1
    ref_stem = RR.conv2d(x, w, b, 2)
    stem, pool = K.resnet_stem_pool(_dev(x), w.cuda(), b.cuda(), want_stem=True)
    assert tuple(stem.shape) == (2, 64, 64, 512) and tuple(pool.shape) == (2, 64, 32, 256)
    assert _rel(stem, ref_stem) < 1e-3
    assert _rel(pool, RR.max_pool(ref_stem)) < 1e-3
    assert torch.equal(pool.cpu(), RR.max_pool(stem.cpu()))              # bit-exact pool of the kernel's own stem
    assert torch.equal(K.max_pool2d(stem).cpu(), pool.cpu())             # the standalone pool kernel: the same values
    _, pool_only = K.resnet_stem_pool(_dev(x), w.cuda(), b.cuda())
    assert torch.equal(pool_only.cpu(), pool.cpu())
    stem16, pool16 = K.resnet_stem_pool(_dev(x, torch.bfloat16), w.cuda(), b.cuda(), want_stem=True)
    assert torch.equal(pool16.cpu(), RR.max_pool(stem16.cpu().float()).bfloat16())
    assert _rel(stem16.float(), ref_stem) < 1e-2


@pytest.mark.parametrize("ci,co,h,w,stride", [(64, 64, 32, 256, 1), (64, 128, 32, 256, 2), (128, 256, 16, 128, 2), (256, 512, 8, 64, 2)])
def test_projection_shortcut(ci, co, h, w, stride):
    g = torch.Generator().manual_seed(2)
    x = torch.randn(2, ci, h, w, generator=g)
    wt = torch.randn(1, 1, ci, co, generator=g) / ci ** 0.5
    y = _K().conv1x1_fwd(_dev(x), wt.cuda(), stride)
    assert tuple(y.shape) == (2, co, h // stride, w // stride)
    assert _rel(y, RR.conv2d(x, wt, None, stride)) < 1e-3


@pytest.mark.parametrize("ci,co,h,w,stride", [(512, 512, 4, 32, 1), (256, 512, 8, 64, 2), (64, 128, 32, 256, 2)])
def test_conv3x3_of_the_classifier(ci, co, h, w, stride):
    """The implicit-GEMM convs at the classifier's widths: 512 channels on 4 x 32 and the stride-2 entries of stages 2-4."""
    K = _K()
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, ci, h, w, generator=g)
    wt = torch.randn(3, 3, ci, co, generator=g) * 0.05
    b = torch.randn(co, generator=g) * 0.1
    from gansynth_amd._lib import GS_F32
    ws = K.conv2d_fwd_workspace((2, ci, h, w), co, 3, stride, GS_F32)
    y = K.conv2d_fwd_bias_ws(_dev(x), _ws_weight(wt), b.cuda(), 3, stride, ws, 0)
    ref = RR.conv2d(x, RR.weight_standardization(wt), b, stride)
    assert _rel(y, ref) < 1e-3
    y2 = K.conv2d_fwd_bias_ws(_dev(x), _ws_weight(wt), b.cuda(), 3, stride, ws, 1)   # the prepared operand reused
    assert torch.equal(y, y2)


@pytest.mark.parametrize("c,h,w", [(64, 32, 256), (128, 16, 128), (256, 8, 64), (512, 4, 32)])
@pytest.mark.parametrize("offset", [0.0, 50.0])
def test_group_norm_relu_every_width(c, h, w, offset):
    """32 groups at every width; offset 50 with a spread of 0.02: |mean| / std = 2500 (a sum of squares would cancel)."""
    K = _K()
    g = torch.Generator().manual_seed(4)
    scale = 0.02 if offset else 1.0
    x = (torch.randn(2, c, h, w, generator=g) * scale + offset + torch.randn(1, c, 1, 1, generator=g) * scale).float()
    gamma, beta = 1.0 + 0.3 * torch.randn(c, generator=g), 0.2 * torch.randn(c, generator=g)
    stats, s = K.group_norm_stats(_dev(x), 32, RR.EPS)
    ref_stats = RR.group_stats(x.double(), 32)
    assert _rel(stats[..., 0], ref_stats[..., 0]) < 1e-4
    assert _rel(stats[..., 1], ref_stats[..., 1]) < 1e-3
    y = K.group_norm_apply(_dev(x), stats, gamma.cuda(), beta.cuda(), relu=True)
    assert _rel(y, torch.relu(RR.group_norm(x.double(), gamma, beta, 32))) < 1e-3
    from gansynth_amd import ops, variables
    old = variables._default
    variables.set_default_store(variables.VariableStore(device="cuda"))
    try:   # ops.group_normalization: the reference's function (no relu), fresh variables (gamma 1, beta 0)
        z = ops.group_normalization(_dev(x), 32)
        assert _rel(z, RR.group_norm(x.double(), torch.ones(c), torch.zeros(c), 32)) < 1e-3
    finally:
        variables._default = old


def test_residual_add_fused_into_the_statistics():
    K = _K()
    g = torch.Generator().manual_seed(5)
    u, sc = torch.randn(2, 256, 8, 64, generator=g), torch.randn(2, 256, 8, 64, generator=g) + 1.0
    stats, s = K.group_norm_stats(_dev(u), 32, RR.EPS, addend=_dev(sc))
    assert torch.equal(s.cpu(), u + sc)                                    # the stored sum: one IEEE add per element
    ref = RR.group_stats((u + sc).double(), 32)
    assert _rel(stats[..., 0], ref[..., 0]) < 1e-5 and _rel(stats[..., 1], ref[..., 1]) < 1e-3
    s16 = K.group_norm_stats(_dev(u, torch.bfloat16), 32, RR.EPS, addend=_dev(sc, torch.bfloat16))[1]
    assert torch.equal(s16.cpu(), (u.bfloat16().float() + sc.bfloat16().float()).bfloat16())


def test_head():
    K = _K()
    g = torch.Generator().manual_seed(6)
    x = torch.randn(3, 512, 4, 32, generator=g) + 0.5
    gamma, beta = 1.0 + 0.3 * torch.randn(512, generator=g), 0.2 * torch.randn(512, generator=g)
    stats, _ = K.group_norm_stats(_dev(x), 32, RR.EPS)
    f = K.group_norm_relu_mean(_dev(x), stats, gamma.cuda(), beta.cuda())
    assert tuple(f.shape) == (3, 512) and f.dtype == torch.float32
    assert _rel(f, torch.relu(RR.group_norm(x.double(), gamma, beta, 32)).mean(dim=(2, 3))) < 1e-3


@pytest.fixture(scope="module")
def full_forward():
    """One batch-2 full-size forward in fp32 and bf16 (random weights, gamma / beta / biases moved off 1 / 0 / 0), and the oracle."""
    from gansynth_amd.networks import ResNet
    net = ResNet.pitch_classifier()
    names = [(k, tuple(v.shape)) for k, v in net.create_variables().items()]
    params = RR.random_params(names, seed=7)
    net.load_state_dict(params)
    g = torch.Generator().manual_seed(8)
    x = torch.randn(2, 2, 128, 1024, generator=g)
    f32 = net(_dev(x))
    f32_again = net(_dev(x))
    bf16 = net(_dev(x, torch.bfloat16))
    ref = RR.forward(params, x)
    return dict(f32=f32, f32_again=f32_again, bf16=bf16, ref=ref)


def test_full_forward_fp32(full_forward):
    (f, l), (rf, rl) = full_forward["f32"], full_forward["ref"]
    assert tuple(f.shape) == (2, 512) and tuple(l.shape) == (2, 61)
    assert _rel(f, rf) < 1e-3, _rel(f, rf)
    assert _rel(l, rl) < 1e-3, _rel(l, rl)


def test_full_forward_bf16(full_forward):
    """bf16 activations (fp32 accumulation, fp32 statistics): each of the ~70 tensors the forward stores (conv outputs, normalised
    activations, residual sums) is rounded to 2^-9 relative, independently, and every group normalisation rescales the error with the
    signal, so it accumulates like a random walk over the 16 blocks rather than growing with depth: sqrt(70) * 2^-9 ~ 3e-2.
    Measured on the MI355X with three weight seeds (profiles/cls_forward_error.json): features 2.1-2.7e-2, logits 1.1-1.4e-3 of their
    largest magnitude (the dense layer averages the feature errors).  Bound: 5e-2 for both."""
    (f, l), (rf, rl) = full_forward["bf16"], full_forward["ref"]
    assert _rel(f, rf) < 5e-2, _rel(f, rf)
    assert _rel(l, rl) < 5e-2, _rel(l, rl)


def test_two_forwards_are_bit_identical(full_forward):
    (f, l), (f2, l2) = full_forward["f32"], full_forward["f32_again"]
    assert torch.equal(f, f2) and torch.equal(l, l2)


# ---------------------------------------------------------------------------------------------------------------- evaluate
def _classifier_file(path, seed=9):
    from gansynth_amd import classifier_io, variables
    from gansynth_amd.networks import ResNet
    net = ResNet.pitch_classifier(store=variables.VariableStore(device="cpu"))
    names = [(k, tuple(v.shape)) for k, v in net.create_variables().items()]
    classifier_io.write_safetensors(str(path), RR.random_params(names, seed=seed))
    return str(path)


def _gan(batch, batches, seed=0):
    from gansynth_amd import variables
    from gansynth_amd.dataset import synthetic_nsynth_input_fn
    from gansynth_amd.models import GANSynth
    from gansynth_amd.networks import PGGAN
    from gansynth_amd.utils import Dict
    from oracle import torch_ref as R
    variables.set_default_store(variables.VariableStore(device="cuda", seed=0))
    pg = PGGAN(min_resolution=[2, 16], max_resolution=[128, 1024], min_channels=32, max_channels=256, growing_level=1.0)
    gen = torch.Generator(device="cuda").manual_seed(seed)
    spectral = Dict(waveform_length=64000, sample_rate=16000, spectrogram_shape=[128, 1024], overlap=0.75)
    real_fn = synthetic_nsynth_input_fn(batch, range(24, 85), num_batches=batches, device=torch.device("cuda"), seed=seed)
    return GANSynth(pg.generator, pg.discriminator, real_fn, lambda: torch.randn(batch, 256, device="cuda", generator=gen), spectral,
                    Dict(R.DEFAULT_HYPER), dtype=torch.float32)


def test_evaluate_returns_the_fid_of_its_features(tmp_path, gpu_store):
    from gansynth_amd import checkpoint, metrics
    from gansynth_amd.networks import ResNet
    clf = _classifier_file(tmp_path / "clf.safetensors")
    model = _gan(32, 32)                                   # 1024 examples per side: the 512 x 512 covariances have full rank
    lat = torch.randn(32, 256, device="cuda")
    model._ensure_built(lat, torch.eye(61, device="cuda")[:32])
    keys = list(checkpoint.state_dict(model).keys())
    checkpoint.save(model, str(tmp_path))
    with pytest.raises(ValueError, match="images:0"):
        model.evaluate(str(tmp_path), None, clf, "input:0", ["features:0", "logits:0"])
    exported = {}
    out = model.evaluate(str(tmp_path), None, clf, "images:0", ["features:0", "logits:0"], features_out=exported, extra_metrics=True)
    assert model.restored_from is not None
    assert exported["real_features"].shape == (1024, 512) and exported["fake_features"].shape == (1024, 512)
    fid = out["frechet_inception_distance"]
    assert np.isfinite(fid) and fid == pytest.approx(metrics.frechet_inception_distance(exported["real_features"], exported["fake_features"]), rel=1e-9)
    assert 1.0 <= out["inception_score"] <= 61.0 and 0.0 <= out["pitch_accuracy"] <= 1.0
    assert list(checkpoint.state_dict(model).keys()) == keys   # the classifier's variables live in its own store

    # the real set against itself through the whole path: a "generator" that returns the batch's own real images
    from gansynth_amd import spectral_ops
    model2 = _gan(32, 32, seed=1)
    model2._ensure_built(lat, torch.eye(61, device="cuda")[:32])
    last = {}
    real_fn = model2.real_input_fn

    def stash():
        data, labels = real_fn()
        last["data"] = data
        return data, labels
    model2.real_input_fn = stash
    model2.generator = lambda latents, labels: spectral_ops.convert_to_images(last["data"].cuda(), **model2.spectral_params)
    net = ResNet.pitch_classifier().load(clf)
    same = {}
    out2 = model2.evaluate(None, None, net, "images:0", ["features:0", "logits:0"], features_out=same)
    assert np.array_equal(same["real_features"], same["fake_features"])
    scale = float(np.trace(np.cov(same["real_features"], rowvar=False)))
    assert abs(out2["frechet_inception_distance"]) < 1e-4 * scale, (out2, scale)


def test_gan_synth_main_evaluate(tmp_path):
    clf = _classifier_file(tmp_path / "clf.safetensors", seed=10)
    cmd = [sys.executable, os.path.join(ROOT, "gan_synth_main.py"), "--evaluate", "--generate", "--synthetic", "--classifier", clf,
           "--model_dir", str(tmp_path / "model"), "--batch_size", "16", "--num_generate_batches", "40"]
    r = subprocess.run(cmd, cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    line = [s for s in r.stdout.splitlines() if "frechet_inception_distance" in s][-1]
    fid = float(line.split(":")[1].strip(" }"))
    assert np.isfinite(fid) and fid >= 0.0, line
    assert len(os.listdir(tmp_path / "samples")) == 640   # --generate after --evaluate: evaluate ran over an input of its own
