"""CPU: the cases of tests/test_classifier_cover_gpu.py exist and mean something (no GPU: the *_workspace_bytes functions of the library are host
arithmetic on the geometry the entry points read).

- On a grid on both sides of every threshold (batches up to 2049, every channel count from 4 to 1024, pixel counts around 4 R k, M around multiples
  of 32, stem tiles around 1024, n / 4 around 1024 and 1024 * 1024) the byte counts the library answers are those the restated geometry of
  classifier_cover implies; S, splits and blocks are recovered from them.
- Every case has every fact in its `want`; the 40 instantiations all have a case; every fact the suite did not see before has one, in each dtype
  that has the kernel.
- The geometry of the layers the real classifier runs at 128 x 1024, batch 8 and 64, is pinned to literals read off the code.
- The float64 references agree to 1e-12 of max |ref| with independently formulated float64 torch, the closed-form group-norm backward with autograd.
- The share of undecided ReLU elements of every group-norm backward case is at most 0.1 %, and 0 where the case has few elements.
- The entry points refuse what they must, with their code and nothing launched."""
import math

import pytest
import torch
import torch.nn.functional as TF

from tests import classifier_cover as C
from tests import resnet_ref as RR

POW2 = (4, 8, 16, 32, 64, 128, 256, 512, 1024)


@pytest.fixture(scope="module")
def lib():
    from gansynth_amd import _lib
    assert (_lib.GS_F32, _lib.GS_BF16) == (C.F32, C.BF16)
    return _lib.load()


# ----------------------------------------------------------------------------------------------------- restatement equals the library
def test_group_norm_geometry_equals_the_library(lib):
    seen, checked = set(), 0
    for n in (1, 2, 3, 7, 8, 64, 1023, 1024, 1025, 2047, 2048, 2049):
        for c in POW2:
            R = 1024 // c
            ks = {1, 2, 3, 5, 8, 2048 // n, 2048 // n + 1, 2 * (2048 // n) + 1} - {0}
            hws = {1, 2, 15, 99} | {4 * R * k + e for k in ks for e in (-1, 0, 1, 3)}
            for hw in sorted(h for h in hws if 0 < h <= 1 << 22):
                S, pps = C.gn_geometry(n, hw, c)
                assert S >= 1 and (S - 1) * pps < hw <= S * pps                   # the slices cover the image and the last one is not empty
                for G in {1, c // min(c, 64), c}:
                    fwd, bwd = lib.gs_group_norm_workspace_bytes(n, hw, c, G), lib.gs_group_norm_bwd_workspace_bytes(n, hw, c, G)
                    assert fwd == C.gn_workspace_bytes(n, hw, c, G) and bwd == C.gn_bwd_workspace_bytes(n, hw, c, G), (n, hw, c, G, fwd, bwd)
                    assert fwd // (n * G * 12) == S and (bwd // 8 - n * c - n * G) // (n * c) == S
                    checked += 1
                seen.add((S == 1, S % 4 != 0, S * pps != hw, hw < R, S == 2048 // n))
    assert checked > 5000 and all(any(s[i] for s in seen) for i in range(5))
    assert lib.gs_group_norm_workspace_bytes(0, 8, 64, 32) == 0 and lib.gs_group_norm_bwd_workspace_bytes(2, 0, 64, 32) == 0


def test_conv1x1_split_equals_the_library(lib):
    seen = set()
    ms = sorted({m + e for m in (32, 64, 96, 512, 544, 558, 16384, 16416, 32768) for e in (-1, 0, 1)} | {1, 30, 70})
    for ci in (64, 128, 256, 512):
        for co in (64, 128, 512):
            for M in ms:
                splits, rows = C.conv1x1_wgrad_split(M, ci, co)
                assert rows % 32 == 0 and (splits - 1) * rows < M <= splits * rows
                for stride, (n, h, w) in ((1, (1, 1, M)), (2, (1, 2, 2 * M)), (1, (M, 1, 1))):
                    got = lib.gs_conv1x1_bwd_weight_workspace_bytes(n, h, w, ci, co, stride)
                    assert got == C.conv1x1_wgrad_workspace_bytes(n, h, w, ci, co, stride) and got // (ci * co * 4) == splits, (M, ci, co, stride, got)
                seen.add((splits == 1, M % rows != 0, M % 64 != 0, splits == 512 // ((ci // 64) * (co // 64))))
    assert all(any(s[i] for s in seen) for i in range(4))
    assert lib.gs_conv1x1_bwd_weight_workspace_bytes(1, 4, 4, 32, 64, 1) == 0 and lib.gs_conv1x1_bwd_weight_workspace_bytes(1, 4, 4, 64, 64, 3) == 0


def test_stem_and_momentum_blocks_equal_the_library(lib):
    capped = set()
    for w in (4, 64, 68, 72, 1024):
        col_tiles = C._cdiv(w // 2, C.STEMB_TW)
        for n in (1, 2, 5):
            for tiles_wanted in (1, 4, 1020, 1022, 1023, 1024, 1025, 1026, 1280, 2048, 2049):
                h = 2 * max(1, tiles_wanted // (n * col_tiles))
                if h % 4:
                    h += 2
                tiles, blocks, trips = C.stem_wgrad_blocks(n, h, w)
                got = lib.gs_resnet_stem_bwd_weight_workspace_bytes(n, h, w)
                assert got == C.stem_wgrad_workspace_bytes(n, h, w) and got // (99 * 64 * 4) == blocks == min(tiles, 1024), (n, h, w, got)
                assert (trips - 1) * blocks < tiles <= trips * blocks
                capped.add((tiles > 1024, tiles == 1024, tiles < 1024))
    assert capped == {(True, False, False), (False, True, False), (False, False, True)}
    assert lib.gs_resnet_stem_bwd_weight_workspace_bytes(0, 4, 4) == 0
    capped = set()
    for n4 in (1, 2, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 1024 * 1023, 1024 * 1024 - 1, 1024 * 1024, 1024 * 1024 + 1, 1024 * 1024 + 37, 5 * 1024 * 1024 + 1):
        blocks, trips = C.momentum_blocks(4 * n4)
        got = lib.gs_momentum_workspace_bytes(4 * n4)
        assert got == C.momentum_workspace_bytes(4 * n4) and got // 8 == blocks and (trips - 1) * blocks * 256 < n4 <= trips * blocks * 256, (n4, got)
        capped.add((blocks == 1, blocks == 1024, trips > 4))
    assert all(any(s[i] for s in capped) for i in range(3))
    assert lib.gs_momentum_workspace_bytes(0) == 0


# ------------------------------------------------------------------------------------------------------- cases mean what they claim
def test_every_case_has_the_facts_it_claims():
    for c in C.CASES:
        f = C.facts(c)
        for k, v in c.want.items():
            assert k in f and f[k] == v, f"{C.case_id(c)}: wants {k}={v}, the geometry gives {k}={f.get(k)}"
        assert c.key in C.case_keys(c), C.case_id(c)
    assert len({C.case_id(c) for c in C.CASES}) == len(C.CASES)


def test_every_instantiation_and_every_unseen_fact_has_a_case():
    assert len(C.KERNELS) == 40
    covered = set().union(*(C.case_keys(c) for c in C.CASES))
    assert covered == set(C.KERNELS), (sorted(map(C.key_id, set(C.KERNELS) - covered)), sorted(map(C.key_id, covered - set(C.KERNELS))))
    assert {c.key for c in C.CASES} <= set(C.KERNELS)
    missing = C.missing_facts()
    assert not missing, "no case reaches: " + "; ".join(missing)
    # the fold: one slice, fewer than its 4 lanes, exactly 4, several trips of a lane, 256 trips
    folds = {C.facts(c)["splits"] for c in C.CASES if c.op == "conv1x1_bwd_weight"} | {C.facts(c)["blocks"] for c in C.CASES if c.op == "stem_wgrad"}
    assert {1, 3, 4, 9, 1024} <= folds, folds


def test_the_numbers_of_the_case_shapes_by_hand():
    """The shapes of the cases and the numbers they were chosen for, written out once more by hand."""
    assert C.gn_geometry(2, 15, 4) == (1, 15) and 1024 // 4 == 256
    assert C.gn_geometry(2, 99, 256) == (6, 17) and 99 - 5 * 17 == 14
    assert C.gn_geometry(1, 18, 1024) == (4, 5) and 18 - 3 * 5 == 3
    assert C.gn_geometry(2, 2097171, 4) == (1024, 2049) and 2 * 2097171 - 16384 * 256 == 38
    assert C.conv1x1_wgrad_split(30, 64, 64) == (1, 32) and C.conv1x1_wgrad_split(70, 64, 64) == (3, 32)
    assert C.conv1x1_wgrad_split(558, 256, 512) == (9, 64) and 558 - 8 * 64 == 46 and C.conv1x1_wgrad_split(1, 128, 64) == (1, 32)
    assert C.stem_wgrad_blocks(2, 4, 4) == (4, 4, 1) and C.stem_wgrad_blocks(1, 12, 72) == (12, 12, 1) and C.stem_wgrad_blocks(5, 512, 4) == (1280, 1024, 2)
    assert C.stem_pool_grid(1, 12, 72) == (2, 2, 1) and C.stem_pool_grid(2, 4, 4) == (1, 1, 2)
    assert C.momentum_blocks(C.MOM_N) == (1024, 5) and C.MOM_N // 4 - 4 * 1024 * 256 == 37
    assert C.grid_stride(64 * 257 * 257, C.POOL_BWD_GRID_CAP) == (16384, 2) and C.grid_stride(64 * 129 * 255, C.POOL_GRID_CAP) == (8192, 2)
    assert {c.shape[:4] for c in C.CASES if c.op == "gn_stats"} == {(2, 4, 3, 5), (2, 32, 5, 7), (2, 256, 9, 11), (1, 1024, 3, 6), (3, 64, 8, 32)}
    assert {c.shape[0] for c in C.CASES if c.op == "softmax_xent"} == {1, 256, 257, 600}
    assert {(c.args["lo"], c.args["hi"]) for c in C.CASES if c.op == "momentum"} == {(0, C.MOM_N), (5, 4 * 1024 * 1024 + 3), (8, 8)}


# -------------------------------------------------------------------------------------------------------- production geometry, pinned
# the classifier at 128 x 1024: (c, h, w) of the group norms of the four stages; (ci, co, stride, h, w) of the projections
_GN_LAYERS = ((64, 32, 256), (128, 16, 128), (256, 8, 64), (512, 4, 32))
_PROJ_LAYERS = ((64, 64, 1, 32, 256), (64, 128, 2, 32, 256), (128, 256, 2, 16, 128), (256, 512, 2, 8, 64))
_MODEL = {   # batch -> what the current code does there
    8: dict(gn=((128, 64), (64, 32), (32, 16), (16, 8)), gn_grid=((4096, 1), (2048, 1), (1024, 1), (512, 1)),
            proj=((512, 128), (256, 64), (64, 64), (16, 64)), stem=(8192, 1024, 8), stem_grid=(16, 16, 8), pool_bwd=(16384, 4), pool=(8192, 2)),
    64: dict(gn=((32, 256), (32, 64), (32, 16), (16, 8)), gn_grid=((16384, 2), (16384, 1), (8192, 1), (4096, 1)),
             proj=((512, 1024), (256, 512), (64, 512), (16, 512)), stem=(65536, 1024, 64), stem_grid=(16, 16, 64), pool_bwd=(16384, 32), pool=(8192, 16)),
}


def test_the_geometry_of_the_model(lib):
    for n, want in _MODEL.items():
        for (c, h, w), sp, grid in zip(_GN_LAYERS, want["gn"], want["gn_grid"]):
            assert C.gn_geometry(n, h * w, c) == sp and C.grid_stride(n * h * w * c // 4, C.GN_GRID_CAP) == grid, (n, c, h, w)
            assert lib.gs_group_norm_workspace_bytes(n, h * w, c, 32) == n * sp[0] * 32 * 12
        for (ci, co, s, h, w), sr in zip(_PROJ_LAYERS, want["proj"]):
            assert C.conv1x1_wgrad_split(n * (h // s) * (w // s), ci, co) == sr, (n, ci, co)
            assert lib.gs_conv1x1_bwd_weight_workspace_bytes(n, h, w, ci, co, s) == sr[0] * ci * co * 4
        assert C.stem_wgrad_blocks(n, 128, 1024) == want["stem"] and C.stem_pool_grid(n, 128, 1024) == want["stem_grid"]
        assert lib.gs_resnet_stem_bwd_weight_workspace_bytes(n, 128, 1024) == 1024 * 99 * 64 * 4
        assert C.grid_stride(n * 64 * 64 * 512, C.POOL_BWD_GRID_CAP) == want["pool_bwd"] and C.grid_stride(n * 64 * 32 * 256, C.POOL_GRID_CAP) == want["pool"]
    # the optimiser walks the classifier's 21.3 million parameters (before the flat buffer's padding) on capped blocks
    assert C.momentum_blocks(21322752) == (1024, 21) and lib.gs_momentum_workspace_bytes(21322752) == 1024 * 8


# --------------------------------------------------------------------------------------------------------------- references are right
def _small(c):
    return not C.is_large(c)


def _close(a, b):
    a, b = a.double(), b.double().reshape(a.shape)
    return float((a - b).abs().max()) <= 1e-12 * float(b.abs().max())


def _independent(c, d):
    """name -> float64 tensor, formulated without tests/resnet_ref.py."""
    a = c.args
    if c.op.startswith("gn_"):
        n, ch, h, w, G = c.shape
        x, gamma, beta = d["x"].double(), d["gamma"].double(), d["beta"].double()
        if c.op == "gn_stats":
            s = (d["x"].float() + d["addend"].float()).to(d["x"].dtype).double() if a["addend"] else x
            var, mean = torch.var_mean(s.reshape(n, G, -1), dim=2, unbiased=False)
            return {"mean": mean, "rstd": torch.rsqrt(var + C.EPS)}
        if c.op == "gn_apply":
            y = TF.group_norm(x, G, gamma, beta, C.EPS)
            return {"y": torch.relu(y) if a["relu"] else y}
        if c.op == "gn_head":
            return {"features": torch.relu(TF.group_norm(x, G, gamma, beta, C.EPS)).mean(dim=(2, 3))}
        xr, gr, br = (t.clone().requires_grad_(True) for t in (x, gamma, beta))
        y = torch.relu(TF.group_norm(xr, G, gr, br, C.EPS))
        if c.op == "gn_bwd":
            y.backward(d["gy"].double())
        else:
            y.mean(dim=(2, 3)).backward(d["gf"].double())
        dx = xr.grad + (d["addend"].double() if a.get("addend") else 0.0)
        return {"dx": dx, "dgamma": gr.grad + (d["dgamma0"].double() if a["accumulate"] else 0.0), "dbeta": br.grad + (d["dbeta0"].double() if a["accumulate"] else 0.0)}
    if c.op.startswith("conv1x1"):
        ci, co, s, n, h, w = c.shape
        wt = d["w"].double().reshape(ci, co)
        if c.op == "conv1x1_fwd":
            return {"y": torch.einsum("nihw,io->nohw", d["x"].double()[:, :, ::s, ::s], wt)}
        gy = d["gy"].double()
        if c.op == "conv1x1_bwd_data":
            gx = torch.zeros(n, ci, h, w, dtype=torch.float64)
            gx[:, :, ::s, ::s] = torch.einsum("nohw,io->nihw", gy, wt)
            return {"gx": gx + (d["out0"].double() if a["out"] else 0.0)}
        gw = torch.einsum("nihw,nohw->io", d["x"].double()[:, :, ::s, ::s], gy).reshape(1, 1, ci, co)
        return {"gw": gw + (d["out0"].double() if a["out"] else 0.0)}
    if c.op in ("stem_pool", "stem_wgrad"):   # TF SAME of a 7x7 / 2 conv on an even size: 2 before, 3 after
        x = TF.pad(d["x"].double(), (2, 3, 2, 3))
        if c.op == "stem_pool":
            stem = TF.conv2d(x, d["w"].double().permute(3, 2, 0, 1), d["bias"].double() if a["bias"] else None, stride=2)
            out = {"stem": stem}
            if a["want_pool"]:   # 3x3 / 2 SAME on an even size: 0 before, 1 after, -inf
                n, ch, hs, ws = stem.shape
                padded = torch.full((n, ch, hs + 1, ws + 1), -math.inf, dtype=torch.float64)
                padded[:, :, :hs, :ws] = stem
                out["pool"] = TF.max_pool2d(padded, 3, 2)
            return out
        wl = torch.zeros(64, 2, 7, 7, dtype=torch.float64, requires_grad=True)
        bl = torch.zeros(64, dtype=torch.float64, requires_grad=True)
        TF.conv2d(x, wl, bl, stride=2).backward(d["gstem"].double())
        gw, gb = wl.grad.permute(2, 3, 1, 0), bl.grad
        return {"gw": gw + (d["gw0"].double() if a["out"] else 0.0), "gb": gb + (d["gb0"].double() if a["out"] else 0.0)}
    if c.op in ("max_pool", "max_pool_bwd"):
        n, ch, h, w = c.shape
        ph, pw = (1 if h % 2 else 0), (1 if w % 2 else 0)    # pads before: 0 on an even size, 1 on an odd one; 1 after in both
        padded = torch.full((n, ch, h + ph + 1, w + pw + 1), -math.inf, dtype=torch.float64)
        xr = d["x"].double().requires_grad_(True)
        padded[:, :, ph:ph + h, pw:pw + w] = xr
        y = TF.max_pool2d(padded, 3, 2)
        if c.op == "max_pool":
            return {"y": y.detach()}
        y.backward(d["gy"].double())
        return {"gx": xr.grad}
    if c.op == "weight_std":
        out = {}
        for i, (w, go) in enumerate(zip(d["w"], d["gout"])):
            w, go = w.double(), go.double()
            var, mean = torch.var_mean(w, dim=(0, 1, 2), unbiased=False, keepdim=True)
            rstd = torch.rsqrt(var + C.EPS)
            wh = (w - mean) * rstd
            out[f"out{i}"], out[f"rstd{i}"] = wh, rstd.flatten()
            out[f"gw{i}"] = (go - go.mean(dim=(0, 1, 2), keepdim=True) - wh * (go * wh).mean(dim=(0, 1, 2), keepdim=True)) * rstd
        return out
    if c.op == "softmax_xent":
        z, y = d["logits"].double(), d["labels"].double()
        lse = torch.logsumexp(z, dim=1, keepdim=True)
        out = {"loss": ((lse - z) * y).sum(dim=1).mean().reshape(1)}
        if a["want_grad"]:
            out["dlogits"] = (torch.exp(z - lse) * y.sum(dim=1, keepdim=True) - y) / z.shape[0]
        return out
    if c.op == "momentum":   # tf.train.MomentumOptimizer with the L2 term of the loss in the gradient, masks in place of slices
        p, g, acc = d["p"].double(), d["g"].double(), d["accum"].double()
        wd, lr, mom = (float(torch.tensor(d[k], dtype=torch.float32)) for k in ("wd", "lr", "momentum"))
        i = torch.arange(p.numel())
        decayed = ((i >= a["lo"]) & (i < a["hi"])).double()
        out = {"l2": (0.5 * (decayed * p * p).sum()).reshape(1)} if a["want_l2"] else {}
        g = g + wd * decayed * p
        acc = mom * acc + g
        out["p"], out["accum"] = p - lr * (g + mom * acc if a["nesterov"] else acc), acc
        return out
    raise AssertionError(c.op)


@pytest.mark.parametrize("op", sorted({c.op for c in C.CASES if _small(c) or c.op == "momentum"}))
def test_references_agree_with_independent_float64(op):
    n = 0
    for c in C.CASES:
        if c.op != op or not (_small(c) or c.op == "momentum"):   # (both dtypes: a bf16 case's operands are rounded before either side reads them)
            continue
        d = C.inputs(c)
        if c.op in ("gn_apply", "gn_head"):
            d["stats"] = RR.group_stats(d["x"].double(), c.shape[4])   # (the case hands the kernel these rounded to fp32)
        ref, other = C.reference(c, d), _independent(c, d)
        for name, t in other.items():
            e = ref[name]
            if e.ref.abs().max() == 0:
                assert t.abs().max() <= 1e-300 or float(t.abs().max()) < 1e-9, (C.case_id(c), name)
                continue
            assert _close(t, e.ref), (C.case_id(c), name, float((t - e.ref.double().reshape(t.shape)).abs().max()), float(e.ref.abs().max()))
            n += 1
        assert {k for k, e in ref.items() if not isinstance(e, C.Exact)} <= set(other), (C.case_id(c), sorted(ref), sorted(other))
        if c.op == "softmax_xent":   # the count: rows 0 and 2 carry two equal maxima, the first wins
            z, y = d["logits"], d["labels"]
            assert c.args["ties"] == 1
            assert z[0, 7] == z[0, 40] == z[0].max() and int(y[0].argmax()) == 7
            hits = sum(int(min(j for j in range(61) if z[r, j] == z[r].max()) == min(j for j in range(61) if y[r, j] == y[r].max())) for r in range(z.shape[0]))
            assert int(ref["correct"].ref) == hits and 0 < hits < z.shape[0] or z.shape[0] == 1
            if c.args["soft"] and z.shape[0] > 1:
                assert abs(float(y[z.shape[0] // 3].sum()) - 0.9) < 1e-3 or z.shape[0] // 3 in (0, 2)
                assert float(y[-1].sum()) == 0.0
        if c.op in ("gn_bwd", "gn_head_bwd"):   # the closed form against autograd
            dx, dgamma, dbeta, pre, up = C.gn_bwd_reference(c, d)
            cx, cg, cb, cpre = C.gn_relu_bwd_closed(d["x"].double(), d["gamma"].double(), d["beta"].double(), up, c.shape[4])
            assert _close(cx, dx) and _close(cg, dgamma) and _close(cb, dbeta) and _close(cpre, pre), C.case_id(c)
    assert n > 0


def test_max_pool_backward_reference_rounds_once_in_bf16():
    """The kernel rounds the sum of up to 4 stored bf16 gradients once, and so does the reference: a float64 sum of the stored values.  On a 3 x 3
    input (pads 1 / 1) whose centre is the largest element all four windows hand it their gradient: 1 + 3 * 2^-9, which no bf16 holds.  Rounded
    once it is 1 + 2^-7; rounded after every add it stays 1, and the bound tells the two apart."""
    c = C.Case("max_pool_bwd", C.BF16, (1, 1, 3, 3), {}, C.Key("max_pool_bwd", C.BF16, None), {})
    x = torch.full((1, 1, 3, 3), 0.5)
    x[0, 0, 1, 1] = 2.0
    gy = torch.tensor([1.0, 2.0 ** -9, 2.0 ** -9, 2.0 ** -9]).reshape(1, 1, 2, 2)
    d = {"x": x.bfloat16(), "gy": gy.bfloat16()}
    assert torch.equal(d["gy"].float(), gy)
    entry = C.reference(c, d)["gx"]
    want = torch.zeros(1, 1, 3, 3, dtype=torch.float64)
    want[0, 0, 1, 1] = 1.0 + 3 * 2.0 ** -9
    assert torch.equal(entry.ref, want)
    once, every_add = want.to(torch.bfloat16), torch.where(want != 0, 1.0, 0.0).to(torch.bfloat16)
    assert float(once[0, 0, 1, 1]) == 1.0 + 2.0 ** -7
    assert C.within(once, entry)[2] and not C.within(every_add, entry)[2]


def test_the_table_of_the_docstring_is_ceilings():
    rows = {}
    for line in C.__doc__.splitlines():
        f = line.split()
        if len(f) == 4 and f[0] in C.CEILINGS:
            rows[f[0]] = tuple(float(v) for v in f[1:])
    assert rows == {k: tuple(float(x) for x in v) for k, v in C.CEILINGS.items()}
    for k, (measured, suite, here) in C.CEILINGS.items():   # 16 times the measurement, rounded up to a power of ten, never above the suite's own
        assert here == min(suite, 10.0 ** math.ceil(math.log10(16 * measured))), k


# -------------------------------------------------------------------------------------------------------------------- ReLU decisions
def test_undecided_relu_elements_are_few():
    n = 0
    for c in C.CASES:
        if c.op not in ("gn_bwd", "gn_head_bwd"):
            continue
        share = C.undecided_share(c)
        elements = math.prod(c.shape[:4])
        assert share <= 1e-3, (C.case_id(c), share)
        if elements < 1000:   # (a single undecided element would already be more than 0.1 %)
            assert share == 0.0, (C.case_id(c), share, elements)
        n += 1
    assert n >= 30


# --------------------------------------------------------------------------------------------------------------------------- refusals
def test_refusals(lib):
    """What the entry points refuse, with their code -- before anything is dereferenced or launched."""
    P, BIG = 0x10000, 1 << 30
    A, W = C.ERR_ARG, C.ERR_WORKSPACE

    def stats(n, hw, c, G, ws=BIG):
        return lib.gs_group_norm_stats(P, None, None, P, n, hw, c, G, 1e-12, C.F32, P, ws, None)

    def apply(n, hw, c, G):
        return lib.gs_group_norm_apply(P, P, P, P, P, n, hw, c, G, 1, C.F32, None)

    def head(n, hw, c, G):
        return lib.gs_group_norm_relu_mean(P, P, P, P, P, n, hw, c, G, C.F32, None)

    def bwd(n, hw, c, G, ws=BIG):
        return lib.gs_group_norm_relu_bwd(P, P, P, P, P, None, P, P, P, n, hw, c, G, 0, C.F32, P, ws, None)

    def head_bwd(n, hw, c, G, ws=BIG):
        return lib.gs_group_norm_relu_mean_bwd(P, P, P, P, P, P, P, P, n, hw, c, G, 0, C.F32, P, ws, None)
    for c, G in ((48, 4), (2048, 32), (2, 1)):   # not a power of two; more than 1024; fewer than 4
        assert stats(2, 64, c, G) == A and b"channels" in lib.gs_last_error()
        assert apply(2, 64, c, G) == A and head(2, 64, c, G) == A and bwd(2, 64, c, G) == A and head_bwd(2, 64, c, G) == A
    assert stats(2, 64, 64, 48) == A and b"groups" in lib.gs_last_error()
    assert bwd(2, 64, 256, 2) == A and b"per group" in lib.gs_last_error() and head_bwd(2, 64, 256, 2) == A      # 128 channels per group
    assert head(2, 64, 32, 32) == A and b"multiple of 64" in lib.gs_last_error()
    assert stats(2, 64, 64, 32, ws=lib.gs_group_norm_workspace_bytes(2, 64, 64, 32) - 1) == W and b"workspace" in lib.gs_last_error()
    short = lib.gs_group_norm_bwd_workspace_bytes(2, 64, 64, 32) - 1
    assert bwd(2, 64, 64, 32, ws=short) == W and head_bwd(2, 64, 64, 32, ws=short) == W and b"workspace" in lib.gs_last_error()
    assert lib.gs_group_norm_stats(P, P, None, P, 2, 64, 64, 32, 1e-12, C.F32, P, BIG, None) == A                # an addend and nowhere to store the sum

    def data(n, h, w, ci, co, s):
        return lib.gs_conv1x1_bwd_data(P, P, P, n, h, w, ci, co, s, 0, C.F32, None)

    def weight(n, h, w, ci, co, s, ws=BIG):
        return lib.gs_conv1x1_bwd_weight(P, P, P, n, h, w, ci, co, s, 0, C.F32, P, ws, None)
    assert data(2, 4, 4, 96, 64, 1) == A and b"multiples of 64" in lib.gs_last_error() and weight(2, 4, 4, 96, 64, 1) == A
    assert data(2, 4, 4, 64, 32, 1) == A and weight(2, 4, 4, 64, 32, 1) == A
    assert lib.gs_conv1x1_fwd(P, P, P, 2, 4, 4, 48, 64, 1, C.F32, None) == A and b"multiples of 32" in lib.gs_last_error()
    for h, w in ((3, 4), (4, 5)):   # stride 2 on an odd size
        assert data(2, h, w, 64, 64, 2) == A and b"stride" in lib.gs_last_error() and weight(2, h, w, 64, 64, 2) == A
        assert lib.gs_conv1x1_fwd(P, P, P, 2, h, w, 64, 64, 2, C.F32, None) == A
    assert data(2, 4, 4, 64, 64, 3) == A
    assert weight(2, 4, 4, 64, 64, 1, ws=lib.gs_conv1x1_bwd_weight_workspace_bytes(2, 4, 4, 64, 64, 1) - 1) == W and b"workspace" in lib.gs_last_error()

    assert lib.gs_resnet_stem_pool(P, P, P, None, P, 2, 6, 8, 64, C.F32, None) == A and b"multiples of 4" in lib.gs_last_error()
    assert lib.gs_resnet_stem_pool(P, P, P, None, P, 2, 8, 6, 64, C.F32, None) == A and lib.gs_resnet_stem_pool(P, P, P, None, None, 2, 8, 8, 64, C.F32, None) == A
    assert lib.gs_resnet_stem_pool(P, P, P, None, P, 2, 8, 8, 32, C.F32, None) == A and b"output channels" in lib.gs_last_error()
    assert lib.gs_resnet_stem_bwd_weight(P, P, P, P, 2, 6, 8, 64, 0, C.F32, P, BIG, None) == A and b"multiples of 4" in lib.gs_last_error()
    assert lib.gs_resnet_stem_bwd_weight(P, P, P, P, 2, 8, 8, 64, 0, C.F32, P, lib.gs_resnet_stem_bwd_weight_workspace_bytes(2, 8, 8) - 1, None) == W
    assert lib.gs_max_pool2d(P, P, 2, 3, 4, 8, C.F32, None) == A and lib.gs_max_pool2d_bwd(P, P, P, 2, 3, 4, 8, 2, None) == A

    def step(n, lo, hi, ws=BIG):
        return lib.gs_momentum_tf_step(P, P, P, n, lo, hi, 0.01, 0.05, 0.9, 1, 1, None, P, ws, None)
    assert step(6, 0, 0) == A and b"multiple of 4" in lib.gs_last_error()
    for lo, hi in ((-1, 4), (0, 9), (5, 4)):   # a decayed range outside the buffer, or backwards
        assert step(8, lo, hi) == A and b"range" in lib.gs_last_error()
    assert step(4096 * 4, 0, 0, ws=lib.gs_momentum_workspace_bytes(4096 * 4) - 1) == W and b"workspace" in lib.gs_last_error()
    assert lib.gs_softmax_xent(P, P, P, None, None, 4, 61, None) == A
