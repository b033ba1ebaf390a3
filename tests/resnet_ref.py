"""Independent float64 torch-CPU restatement of the pitch classifier (reference networks.py:293-413, ops.py:53-66,120-146,221-247,
308-316): the oracle of tests/test_classifier_gpu.py.  NCHW tensors, HWIO weights; TF SAME padding written out (pad total
max((ceil(n / s) - 1) s + k - n, 0), the smaller half before), -inf padding for the max pool, population variances."""
import math

import numpy as np
import torch
import torch.nn.functional as TF

EPS = 1.0e-12


def same_pads(n, k, s):
    out = -(-n // s)
    total = max((out - 1) * s + k - n, 0)
    return total // 2, total - total // 2


def weight_standardization(w, eps=EPS):
    w = torch.as_tensor(w, dtype=torch.float64)
    axes = tuple(range(w.dim() - 1))
    mean = w.mean(dim=axes, keepdim=True)
    var = ((w - mean) ** 2).mean(dim=axes, keepdim=True)
    return (w - mean) / torch.sqrt(var + eps)


def conv2d(x, w_hwio, bias, stride):
    x = torch.as_tensor(x, dtype=torch.float64)
    w = torch.as_tensor(w_hwio, dtype=torch.float64)
    k = w.shape[0]
    ph, pw = same_pads(x.shape[2], k, stride), same_pads(x.shape[3], k, stride)
    y = TF.conv2d(TF.pad(x, (pw[0], pw[1], ph[0], ph[1])), w.permute(3, 2, 0, 1), stride=stride)
    if bias is not None:
        y = y + torch.as_tensor(bias, dtype=torch.float64).view(1, -1, 1, 1)
    return y


def max_pool(x, k=3, s=2):
    x = torch.as_tensor(x)
    ph, pw = same_pads(x.shape[2], k, s), same_pads(x.shape[3], k, s)
    return TF.max_pool2d(TF.pad(x, (pw[0], pw[1], ph[0], ph[1]), value=-math.inf), k, s)


def group_norm(x, gamma, beta, groups, eps=EPS):
    x = torch.as_tensor(x, dtype=torch.float64)
    n, c, h, w = x.shape
    xr = x.reshape(n, groups, c // groups, h, w)
    mean = xr.mean(dim=(2, 3, 4), keepdim=True)
    var = ((xr - mean) ** 2).mean(dim=(2, 3, 4), keepdim=True)
    y = ((xr - mean) / torch.sqrt(var + eps)).reshape(n, c, h, w)
    return y * torch.as_tensor(gamma, dtype=torch.float64).view(1, c, 1, 1) + torch.as_tensor(beta, dtype=torch.float64).view(1, c, 1, 1)


def group_stats(x, groups, eps=EPS):
    """[n, groups, 2] = (mean, 1 / sqrt(var + eps))."""
    x = torch.as_tensor(x, dtype=torch.float64)
    n, c, h, w = x.shape
    xr = x.reshape(n, groups, -1)
    mean = xr.mean(dim=2)
    var = ((xr - mean[:, :, None]) ** 2).mean(dim=2)
    return torch.stack([mean, 1.0 / torch.sqrt(var + eps)], dim=2)


STAGES = [(64, 1, 3), (128, 2, 4), (256, 2, 6), (512, 2, 3)]   # pitch_classifier_main.py:42-47: (filters, stride, blocks)


def forward(params, x, stages=STAGES, groups=32):
    """(features [n, 512], logits [n, classes]) in float64; params: {variable name: array}."""
    p = {k: torch.as_tensor(np.asarray(v), dtype=torch.float64) for k, v in params.items()}
    x = conv2d(x, weight_standardization(p["resnet/conv/weight"]), p["resnet/conv/bias"], 2)
    x = max_pool(x)
    for i, (filters, stride, blocks) in enumerate(stages):
        for j in range(blocks):
            s = stride if j == 0 else 1
            b = f"resnet/residual_block_{i}_{j}/"
            shortcut = x
            a = torch.relu(group_norm(x, p[b + "group_normalization_1st/gamma"].flatten(), p[b + "group_normalization_1st/beta"].flatten(), groups))
            if j == 0:
                shortcut = conv2d(a, weight_standardization(p[b + "projection_shortcut/weight"]), None, s)
            t = conv2d(a, weight_standardization(p[b + "conv_1st/weight"]), p[b + "conv_1st/bias"], s)
            t = torch.relu(group_norm(t, p[b + "group_normalization_2nd/gamma"].flatten(), p[b + "group_normalization_2nd/beta"].flatten(), groups))
            t = conv2d(t, weight_standardization(p[b + "conv_2nd/weight"]), p[b + "conv_2nd/bias"], 1)
            x = t + shortcut
    x = torch.relu(group_norm(x, p["resnet/group_normalization/gamma"].flatten(), p["resnet/group_normalization/beta"].flatten(), groups))
    features = x.mean(dim=(2, 3))
    logits = features @ p["resnet/logits/weight"] + p["resnet/logits/bias"]
    return features, logits


def random_params(names_shapes, seed=0):
    """Random weights with gamma, beta and biases moved away from their initial values (1, 0, 0)."""
    rng = np.random.default_rng(seed)
    out = {}
    for name, shape in names_shapes:
        if name.endswith("/gamma"):
            v = 1.0 + 0.3 * rng.standard_normal(shape)
        elif name.endswith("/beta") or name.endswith("/bias"):
            v = 0.2 * rng.standard_normal(shape)
        else:
            fan = int(np.prod(shape[:-1]))
            v = rng.standard_normal(shape) * np.sqrt(2.0 / fan) + 0.05 * rng.standard_normal(shape[-1])   # a per-channel mean for WS to remove
        out[name] = v.astype(np.float32)
    return out
