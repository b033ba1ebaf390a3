"""GPU: training the pitch classifier (gansynth_amd/csrc/classifier_bwd.hip, networks.ResNet.forward_backward, models.PitchClassifier.train,
pitch_classifier_main.py) against float64 torch autograd over the building blocks of tests/resnet_ref.py.

Tolerance: 1e-3 of the reference's largest magnitude, per tensor, in fp32 (a float32 restatement of group norm + ReLU backward sits at
1-2e-7 of the float64 one at these shapes: the bound is a ceiling with room).  ReLU decision points: a pre-activation within rounding
of zero may take the other branch on the device and move one gradient element by O(|g|), so the element-wise dx comparison leaves out
the elements whose float64 pre-activation has |y| < 1e-5 max|y|; their share is asserted to stay below 0.1 %.  dgamma, dbeta and every
weight gradient are compared whole."""
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
TOL = 1e-3


def _K():
    from gansynth_amd import kernels
    return kernels.get()


def _dev(t):
    t = torch.as_tensor(t).to("cuda", torch.float32)
    return t.contiguous(memory_format=CL) if t.dim() == 4 else t.contiguous()


def _rel(got, ref, keep=None):
    got = torch.as_tensor(got).detach().double().cpu().reshape(ref.shape)
    ref = torch.as_tensor(ref).detach().double()
    d = (got - ref).abs()
    if keep is not None:
        d = d[keep]
    return float(d.max() / ref.abs().max())


def _leaf(t):
    return t.double().clone().requires_grad_(True)


def _decided(y):
    """Elements whose ReLU decision is not within rounding of zero; their complement's share is bounded."""
    keep = y.detach().abs() >= 1e-5 * y.detach().abs().max()
    assert 1.0 - float(keep.double().mean()) <= 1e-3
    return keep


# ------------------------------------------------------------------------------------------------------------ group norm + ReLU
def _gn_inputs(c, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(2, c, h, w, generator=g) + torch.randn(1, c, 1, 1, generator=g)
    gamma, beta = 1.0 + 0.3 * torch.randn(c, generator=g), 0.2 * torch.randn(c, generator=g)
    gy = torch.randn(2, c, h, w, generator=g)
    addend = torch.randn(2, c, h, w, generator=g)
    return x, gamma, beta, gy, addend


@pytest.mark.parametrize("with_addend", [False, True])
@pytest.mark.parametrize("c,h,w", [(64, 8, 32), (128, 16, 128), (512, 4, 32)])
def test_group_norm_relu_backward(c, h, w, with_addend):
    K = _K()
    x, gamma, beta, gy, addend = _gn_inputs(c, h, w, seed=c + h)
    xr, gr, br = _leaf(x), _leaf(gamma), _leaf(beta)
    pre = RR.group_norm(xr, gr, br, 32)
    torch.relu(pre).backward(gy.double())
    ref_dx = xr.grad + (addend.double() if with_addend else 0.0)
    stats, _ = K.group_norm_stats(_dev(x), 32, RR.EPS)
    dx, dgamma, dbeta = K.group_norm_relu_bwd(_dev(x), stats, gamma.cuda(), beta.cuda(), _dev(gy), addend=_dev(addend) if with_addend else None)
    errs = _rel(dx, ref_dx, _decided(pre)), _rel(dgamma, gr.grad), _rel(dbeta, br.grad)
    print("group_norm_relu_bwd", (c, h, w), with_addend, errs)
    assert max(errs) < TOL, errs
    dx2, dgamma2, dbeta2 = K.group_norm_relu_bwd(_dev(x), stats, gamma.cuda(), beta.cuda(), _dev(gy), addend=_dev(addend) if with_addend else None)
    assert torch.equal(dx, dx2) and torch.equal(dgamma, dgamma2) and torch.equal(dbeta, dbeta2)


def test_head_backward():
    K = _K()
    x, gamma, beta, _, _ = _gn_inputs(512, 4, 32, seed=11)
    gf = torch.randn(2, 512, generator=torch.Generator().manual_seed(12))
    xr, gr, br = _leaf(x), _leaf(gamma), _leaf(beta)
    pre = RR.group_norm(xr, gr, br, 32)
    torch.relu(pre).mean(dim=(2, 3)).backward(gf.double())
    stats, _ = K.group_norm_stats(_dev(x), 32, RR.EPS)
    dx, dgamma, dbeta = K.group_norm_relu_mean_bwd(_dev(x), stats, gamma.cuda(), beta.cuda(), gf.cuda())
    errs = _rel(dx, xr.grad, _decided(pre)), _rel(dgamma, gr.grad), _rel(dbeta, br.grad)
    print("group_norm_relu_mean_bwd", errs)
    assert max(errs) < TOL, errs


# ------------------------------------------------------------------------------------------------------ weight standardisation
WS_SHAPES = [(7, 7, 2, 64), (3, 3, 64, 128), (1, 1, 256, 512), (3, 3, 512, 512)]


def test_weight_standardization_batched_forward_and_backward():
    K = _K()
    g = torch.Generator().manual_seed(20)
    ws = [torch.randn(s, generator=g) * 0.05 + torch.randn(s[-1], generator=g) * 0.3 for s in WS_SHAPES]   # per-channel offsets
    gouts = [torch.randn(s, generator=g) for s in WS_SHAPES]
    rows = []
    for w, go in zip(ws, gouts):
        wd = w.cuda()
        rows.append((wd, torch.empty_like(wd), torch.empty(w.shape[-1], device="cuda"), go.cuda(), torch.empty_like(wd)))
    table = K.weight_standardize_table(rows)
    K.weight_standardize_batch(table, RR.EPS)
    for (wd, out, rstd, gout, gw), w in zip(rows, ws):
        assert torch.equal(out, K.weight_standardize(wd, RR.EPS)), tuple(w.shape)        # bit for bit the per-weight launch
    K.weight_standardize_bwd_batch(table)
    for (wd, out, rstd, gout, gw), w, go in zip(rows, ws, gouts):
        wr = _leaf(w)
        RR.weight_standardization(wr).backward(go.double())
        err = _rel(gw, wr.grad)
        print("weight_standardize_bwd", tuple(w.shape), err)
        assert err < TOL, (tuple(w.shape), err)
        assert not gout.any()                                                             # cleared behind the read


# --------------------------------------------------------------------------------------------------------------- stem and pool
@pytest.mark.parametrize("shape", [(2, 64, 8, 32), (2, 64, 7, 31)])
def test_max_pool_backward(shape):
    g = torch.Generator().manual_seed(30)
    x = torch.randn(shape, generator=g)
    xr = _leaf(x)
    y = RR.max_pool(xr)
    gy = torch.randn(y.shape, generator=g)
    y.backward(gy.double())
    gx = _K().max_pool2d_bwd(_dev(x), _dev(gy))
    assert _rel(gx, xr.grad) < 1e-6      # gradients are moved, and where windows share their maximum, added (up to 4 fp32 adds)
    assert torch.equal((gx != 0).cpu(), xr.grad != 0)


@pytest.mark.parametrize("shape", [(2, 64, 8, 32), (2, 64, 7, 31)])
def test_max_pool_backward_with_ties(shape):
    """Three-level inputs: almost every window has equal maxima, and the gradient goes to the first in row-major window order."""
    g = torch.Generator().manual_seed(32)
    x = torch.randint(0, 3, shape, generator=g).float()
    xr = _leaf(x)
    y = RR.max_pool(xr)
    gy = torch.randn(y.shape, generator=g)
    y.backward(gy.double())
    gx = _K().max_pool2d_bwd(_dev(x), _dev(gy))
    assert _rel(gx, xr.grad) < 1e-6
    assert torch.equal((gx != 0).cpu(), xr.grad != 0)


def test_max_pool_backward_of_a_constant_input():
    """Every element of a window is its maximum: the window's gradient lands on its first in-bounds element -- (2 oy, 2 ox) on an even
    size (pads 0 / 1), and on an odd size (pads 1 / 1) row 0 / column 0 for the first window, 2 o - 1 after it.  Written out by hand."""
    K = _K()
    g = torch.Generator().manual_seed(33)
    gy = torch.randn(2, 64, 4, 16, generator=g)
    want = torch.zeros(2, 64, 8, 32)
    want[:, :, 0::2, 0::2] = gy
    assert torch.equal(K.max_pool2d_bwd(_dev(torch.full((2, 64, 8, 32), 0.5)), _dev(gy)).cpu(), want)
    want = torch.zeros(2, 64, 7, 31)
    rows, cols = [0, 1, 3, 5], [0] + list(range(1, 31, 2))
    want[:, :, torch.tensor(rows)[:, None], torch.tensor(cols)[None, :]] = gy
    assert torch.equal(K.max_pool2d_bwd(_dev(torch.full((2, 64, 7, 31), 0.5)), _dev(gy)).cpu(), want)


@pytest.mark.parametrize("n,h,w", [(2, 32, 128), (1, 128, 1024)])
def test_stem_and_pool_backward(n, h, w):
    """2 x 2 x 32 x 128 pins the 2 / 3 pads of the stem and the 0 / 1 pads of the pool; once at the full 128 x 1024."""
    K = _K()
    g = torch.Generator().manual_seed(31)
    x = torch.randn(n, 2, h, w, generator=g)
    wt = torch.randn(7, 7, 2, 64, generator=g) * 0.2
    b = torch.randn(64, generator=g) * 0.1
    gp = torch.randn(n, 64, h // 4, w // 4, generator=g)
    wr, br = _leaf(wt), _leaf(b)
    RR.max_pool(RR.conv2d(x, wr, br, 2)).backward(gp.double())
    stem, pool = K.resnet_stem_pool(_dev(x), wt.cuda(), b.cuda(), want_stem=True)
    dstem = K.max_pool2d_bwd(stem, _dev(gp))
    gw, gb = K.resnet_stem_bwd_weight(_dev(x), dstem)
    errs = _rel(gw, wr.grad), _rel(gb, br.grad)
    print("stem_pool_bwd", (n, h, w), errs)
    assert max(errs) < TOL, errs
    gw2, gb2 = K.resnet_stem_bwd_weight(_dev(x), dstem)
    assert torch.equal(gw, gw2) and torch.equal(gb, gb2)


# ------------------------------------------------------------------------------------------------------------------ the convs
@pytest.mark.parametrize("ci,co,stride,h,w", [(64, 64, 1, 8, 32), (64, 128, 2, 8, 32), (256, 512, 2, 8, 64)])
def test_projection_backward(ci, co, stride, h, w):
    K = _K()
    g = torch.Generator().manual_seed(40)
    x = torch.randn(2, ci, h, w, generator=g)
    wt = torch.randn(1, 1, ci, co, generator=g) / ci ** 0.5
    gy = torch.randn(2, co, h // stride, w // stride, generator=g)
    other = torch.randn(2, ci, h, w, generator=g)
    xr, wr = _leaf(x), _leaf(wt)
    RR.conv2d(xr, wr, None, stride).backward(gy.double())
    gx = K.conv1x1_bwd_data(_dev(gy), wt.cuda(), (2, ci, h, w), stride)
    gw = K.conv1x1_bwd_weight(_dev(x), _dev(gy), stride)
    into = _dev(other).clone(memory_format=torch.preserve_format)
    K.conv1x1_bwd_data(_dev(gy), wt.cuda(), (2, ci, h, w), stride, out=into)              # added into the other consumer's gradient
    errs = _rel(gx, xr.grad), _rel(gw, wr.grad), _rel(into, xr.grad + other.double())
    print("conv1x1_bwd", (ci, co, stride), errs)
    assert max(errs) < TOL, errs


@pytest.mark.parametrize("ci,co,stride,h,w", [(64, 128, 2, 8, 32), (512, 512, 1, 4, 32)])
def test_conv3x3_backward_at_the_classifier_widths(ci, co, stride, h, w):
    """The existing implicit-GEMM entries on a standardised weight with alpha = 1, the bias gradient from the same launches."""
    K = _K()
    g = torch.Generator().manual_seed(41)
    x = torch.randn(2, ci, h, w, generator=g)
    wt = RR.weight_standardization(torch.randn(3, 3, ci, co, generator=g) * 0.05).float()
    gy = torch.randn(2, co, h // stride, w // stride, generator=g)
    xr, wr, br = _leaf(x), _leaf(wt), _leaf(torch.zeros(co))
    RR.conv2d(xr, wr, br, stride).backward(gy.double())
    gx = K.conv2d_bwd_data(_dev(gy), wt.cuda(), (2, ci, h, w), 3, stride, 1.0)
    gw, gb = torch.zeros(3, 3, ci, co, device="cuda"), torch.zeros(co, device="cuda")
    K.conv2d_bwd_weight(_dev(x), _dev(gy), 3, stride, 1.0, out=gw, bias_out=gb)
    errs = _rel(gx, xr.grad), _rel(gw, wr.grad), _rel(gb, br.grad)
    print("conv3x3_bwd", (ci, co, stride), errs)
    assert max(errs) < TOL, errs


# ------------------------------------------------------------------------------------------------------ loss and optimiser
def test_softmax_cross_entropy():
    g = torch.Generator().manual_seed(50)
    logits = torch.randn(5, 61, generator=g) * 3.0
    logits[2] = torch.linspace(-80.0, 80.0, 61)[torch.randperm(61, generator=g)]            # a +-80 spread: no overflow
    target = torch.tensor([3, 60, int(logits[2].argmax()), 0, 17])
    target[0] = int(logits[0].argmax())                                                     # rows 0 and 2 are hits ...
    for r in (1, 3, 4):                                                                     # ... the others are not
        if int(logits[r].argmax()) == int(target[r]):
            target[r] = (target[r] + 1) % 61
    onehot = torch.eye(61)[target]
    zr = _leaf(logits)
    ref = -(torch.log_softmax(zr, dim=1) * onehot.double()).sum(dim=1).mean()
    ref.backward()
    loss, dlogits, correct = _K().softmax_xent(logits.cuda(), onehot.cuda())
    assert abs(float(loss) - float(ref.detach())) < TOL * abs(float(ref.detach()))
    assert _rel(dlogits, zr.grad) < TOL
    assert int(correct) == 2


def _momentum_ref(p, g, a, lo, hi, wd, lr, mom, nesterov):
    g = g.copy()
    l2 = 0.5 * float((p[lo:hi] ** 2).sum())
    g[lo:hi] += wd * p[lo:hi]
    a = mom * a + g
    p = p - (lr * g + lr * mom * a if nesterov else lr * a)
    return p, a, l2


@pytest.mark.parametrize("nesterov", [True, False])
def test_momentum_step(nesterov):
    from gansynth_amd.flat_params import _FlatParams
    from gansynth_amd.models import exponential_decay
    K = _K()
    lr_fn = lambda step: exponential_decay(0.05, step, 2.0, 0.1)
    wd, mom = 1e-2, 0.9

    def run():
        g = torch.Generator().manual_seed(60)
        named = [(k, torch.nn.Parameter(torch.randn(s, generator=g).cuda())) for k, s in (("a/weight", (3, 3, 5, 7)), ("a/bias", (7,)), ("n/gamma", (1, 9, 1, 1)))]
        flat = _FlatParams(named)
        hi = flat._offsets[2][0]                                 # the first two variables are decayed
        p, a = flat.flat.double().cpu().numpy(), np.zeros(flat.flat.numel())
        l2s = []
        for step in range(3):
            grad = torch.randn(flat.flat.numel(), generator=g)
            flat.grad.copy_(grad)
            l2 = K.momentum_tf_step(flat.flat, flat.grad, flat.m, lr_fn(step), mom, nesterov, weight_decay=wd, decay_range=(0, hi))
            p, a, ref_l2 = _momentum_ref(p, grad.double().numpy(), a, 0, hi, wd, lr_fn(step), mom, nesterov)
            assert abs(float(l2) - ref_l2) <= 1e-6 * ref_l2
            assert not flat.grad.any()
            l2s.append(float(l2))
        assert _rel(flat.flat, torch.from_numpy(p)) < TOL and _rel(flat.m, torch.from_numpy(a)) < TOL
        assert torch.equal(named[1][1].data, flat.flat[flat._offsets[1][0]:flat._offsets[1][0] + 7])     # the variables are views
        return flat.flat.clone(), flat.m.clone(), l2s

    first, second = run(), run()
    assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1]) and first[2] == second[2]


# -------------------------------------------------------------------------------------------------- the whole network, reduced
STAGES = [(64, 1, 2), (128, 2, 1)]
HYPER = dict(weight_decay=1e-2, learning_rate=lambda step: 0.05 * 0.5 ** step, momentum=0.9, use_nesterov=True)


def _reduced_net():
    from gansynth_amd import variables
    from gansynth_amd.networks import ResNet
    from gansynth_amd.utils import Dict
    return ResNet(conv_param=Dict(filters=64, kernel_size=[7, 7], strides=[2, 2]), pool_param=Dict(kernel_size=[3, 3], strides=[2, 2]),
                  residual_params=[Dict(filters=f, strides=[s, s], blocks=b) for f, s, b in STAGES], groups=32, classes=61,
                  store=variables.VariableStore(device="cuda", seed=0))


def _ref_loss(p, x, onehot):
    """Mean cross-entropy of the float64 network composed from the differentiable blocks of resnet_ref (p: {name: tensor})."""
    t = RR.max_pool(RR.conv2d(x.double(), RR.weight_standardization(p["resnet/conv/weight"]), p["resnet/conv/bias"], 2))
    for i, (filters, stride, blocks) in enumerate(STAGES):
        for j in range(blocks):
            s = stride if j == 0 else 1
            b = f"resnet/residual_block_{i}_{j}/"
            shortcut = t
            a = torch.relu(RR.group_norm(t, p[b + "group_normalization_1st/gamma"].flatten(), p[b + "group_normalization_1st/beta"].flatten(), 32))
            if j == 0:
                shortcut = RR.conv2d(a, RR.weight_standardization(p[b + "projection_shortcut/weight"]), None, s)
            u = RR.conv2d(a, RR.weight_standardization(p[b + "conv_1st/weight"]), p[b + "conv_1st/bias"], s)
            u = torch.relu(RR.group_norm(u, p[b + "group_normalization_2nd/gamma"].flatten(), p[b + "group_normalization_2nd/beta"].flatten(), 32))
            t = RR.conv2d(u, RR.weight_standardization(p[b + "conv_2nd/weight"]), p[b + "conv_2nd/bias"], 1) + shortcut
    t = torch.relu(RR.group_norm(t, p["resnet/group_normalization/gamma"].flatten(), p["resnet/group_normalization/beta"].flatten(), 32))
    logits = t.mean(dim=(2, 3)) @ p["resnet/logits/weight"] + p["resnet/logits/bias"]
    return -(torch.log_softmax(logits, dim=1) * onehot.double()).sum(dim=1).mean()


def _batches(count, seed=70):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(2, 2, 32, 128, generator=g), torch.eye(61)[torch.randint(0, 61, (2,), generator=g)]) for _ in range(count)]


@pytest.fixture(scope="module")
def reduced():
    """Gradients of one pass and the parameters after three optimiser steps, on the device (twice) and in float64."""
    from gansynth_amd.networks import ResNet
    batches = _batches(3)

    def device_run():
        net = _reduced_net()
        names = [(k, tuple(v.shape)) for k, v in net.create_variables().items()]
        params = RR.random_params(names, seed=71)
        net.load_state_dict(params)
        x, y = batches[0]
        loss, correct, features, logits = net.forward_backward(_dev(x), y.cuda())
        grads = {k: v.grad.detach().cpu().clone() for k, v in net.store.variables.items()}
        for step, (x, y) in enumerate(batches):
            net.forward_backward(_dev(x), y.cuda())
            net.momentum_step(HYPER["learning_rate"](step), HYPER["momentum"], HYPER["use_nesterov"], HYPER["weight_decay"])
        after = {k: v.data.detach().cpu().clone() for k, v in net.store.variables.items()}
        return dict(params=params, loss=float(loss), logits=logits.cpu(), grads=grads, after=after, decayed=ResNet.is_decayed)

    first, second = device_run(), device_run()
    p = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in first["params"].items()}
    ref_loss = _ref_loss(p, *batches[0])
    ref_loss.backward()
    ref_grads = {k: v.grad.clone() for k, v in p.items()}
    vals = {k: v.detach().numpy().copy() for k, v in p.items()}
    acc = {k: np.zeros_like(v) for k, v in vals.items()}
    for step, (x, y) in enumerate(batches):
        q = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in vals.items()}
        _ref_loss(q, x, y).backward()
        for k in vals:
            hi = vals[k].size if first["decayed"](k) else 0
            new, a, _ = _momentum_ref(vals[k].reshape(-1), q[k].grad.numpy().reshape(-1), acc[k].reshape(-1), 0, hi, HYPER["weight_decay"],
                                      HYPER["learning_rate"](step), HYPER["momentum"], HYPER["use_nesterov"])
            vals[k], acc[k] = new.reshape(vals[k].shape), a.reshape(vals[k].shape)
    return dict(first=first, second=second, ref_loss=float(ref_loss), ref_grads=ref_grads, ref_after=vals)


def test_reduced_network_loss_and_gradients(reduced):
    got = reduced["first"]
    assert abs(got["loss"] - reduced["ref_loss"]) < TOL * abs(reduced["ref_loss"]), (got["loss"], reduced["ref_loss"])
    errs = {k: _rel(got["grads"][k], ref) for k, ref in reduced["ref_grads"].items()}
    print("reduced network, worst gradient tensors:", sorted(errs.items(), key=lambda kv: -kv[1])[:4])
    assert len(errs) == len(got["grads"]) and max(errs.values()) < TOL, {k: e for k, e in errs.items() if e >= TOL}


def test_reduced_network_three_steps(reduced):
    errs = {k: _rel(reduced["first"]["after"][k], torch.from_numpy(ref)) for k, ref in reduced["ref_after"].items()}
    print("reduced network after 3 steps, worst variables:", sorted(errs.items(), key=lambda kv: -kv[1])[:4])
    assert max(errs.values()) < TOL, {k: e for k, e in errs.items() if e >= TOL}
    moved = max(float((reduced["first"]["after"][k] - torch.as_tensor(v)).abs().max()) for k, v in reduced["first"]["params"].items())
    assert moved > 1e-3                                                   # (the steps did something)


def test_reduced_network_is_deterministic(reduced):
    a, b = reduced["first"], reduced["second"]
    assert a["loss"] == b["loss"]
    for k in a["after"]:
        assert torch.equal(a["grads"][k], b["grads"][k]) and torch.equal(a["after"][k], b["after"][k]), k


def test_a_pass_after_an_interrupted_one_starts_clean(reduced):
    """A pass that raised part-way leaves partial sums in the standardised weights' gradient buffer: the next one must not add onto them."""
    net = _reduced_net()
    net.load_state_dict(reduced["first"]["params"])
    x, y = _batches(3)[0]
    st = net.train_state()
    st.gstd.fill_(1.0)
    st.gstd_clean = False
    st.flat.grad.fill_(1.0)
    st.flat.grad_clean = False
    net.forward_backward(_dev(x), y.cuda())
    for k, v in net.store.variables.items():
        assert torch.equal(v.grad.cpu(), reduced["first"]["grads"][k]), k


def test_forward_backward_refuses_bf16():
    net = _reduced_net()
    x, y = _batches(1)[0]
    with pytest.raises(TypeError, match="fp32"):
        net.forward_backward(_dev(x).bfloat16(), y.cuda())


# --------------------------------------------------------------------------------------------------------- PitchClassifier.train
def _classifier(seed=80, batches=None):
    from gansynth_amd.models import PitchClassifier
    from gansynth_amd.utils import Dict
    g = torch.Generator().manual_seed(seed)
    left = [batches]

    def input_fn():
        if left[0] is not None:
            if left[0] == 0:
                raise StopIteration
            left[0] -= 1
        return torch.randn(2, 2, 32, 128, generator=g).cuda(), torch.eye(61)[torch.randint(0, 61, (2,), generator=g)].cuda()

    return PitchClassifier(_reduced_net(), input_fn, None, Dict(HYPER))


def test_train_resumes_bit_identically(tmp_path):
    from gansynth_amd import checkpoint
    lines = []
    whole = _classifier()
    whole.train(str(tmp_path / "whole"), None, 6, 2, 100, 1, log=lines.append)
    assert whole.global_step == 6 and len(lines) == 6 and "loss" in lines[0] and "accuracy" in lines[0] and "global_step = 1," in lines[0]
    first = _classifier()
    first.train(str(tmp_path / "split"), None, 4, 2, 100, 100, log=None)
    assert sorted(os.listdir(tmp_path / "split")) == ["checkpoint", "model.ckpt-2.safetensors", "model.ckpt-4.safetensors"]
    resumed = _classifier()
    for _ in range(4):                                                    # the input resumes where the first run stopped
        resumed.input_fn()
    resumed.train(str(tmp_path / "split"), None, 6, 2, 100, 100, log=None)
    assert resumed.global_step == 6 and resumed.restored_from.endswith("model.ckpt-4.safetensors")
    a, b = whole.state_dict(), resumed.state_dict()
    assert list(a) == list(b) and any(k.startswith("momentum/resnet/") for k in a)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert any(np.abs(a[k]).max() > 0 for k in a if k.startswith("momentum/"))
    # a checkpoint is itself a classifier weight file
    path = checkpoint.latest(str(tmp_path / "whole"))
    x = torch.randn(2, 2, 32, 128, generator=torch.Generator().manual_seed(81)).cuda().contiguous(memory_format=CL)
    trained = whole.network(x)
    loaded = _reduced_net().load(path)(x)
    assert torch.equal(trained[0], loaded[0]) and torch.equal(trained[1], loaded[1])
    out = _classifier(batches=3).evaluate(model_dir=str(tmp_path / "whole"))
    assert 0.0 <= out["accuracy"] <= 1.0


def test_pitch_classifier_main_trains(tmp_path):
    cmd = [sys.executable, os.path.join(ROOT, "pitch_classifier_main.py"), "--train", "--synthetic", "--total_steps", "2", "--batch_size", "2",
           "--model_dir", str(tmp_path / "model"), "--log_tensor_steps", "1"]
    r = subprocess.run(cmd, cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "global_step = 2" in r.stdout and os.path.exists(tmp_path / "model" / "model.ckpt-2.safetensors")
