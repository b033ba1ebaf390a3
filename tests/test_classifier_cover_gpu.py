"""GPU: every kernel of csrc/classifier.hip and csrc/classifier_bwd.hip -- all 40 compiled instantiations, at the tile tails, ragged slices,
grid-stride trips, flags and optional arguments of tests/classifier_cover.py -- against float64 on the operands as stored.

One test per case.  It first holds the case's `want` against the geometry the library answers for its shape (the workspace byte counts), so no
case passes at a neighbouring shape; then it runs the case twice through its public entry point (gansynth_amd.kernels; ctypes only for
accumulate = 1 of the group-norm backward, which no wrapper passes), asserts the two runs bit-identical, prints `CLASSIFIER-COVER <case> <result>
ratio ...` and asserts the bound of classifier_cover (run with -s).

test_small_cases_at_the_other_seeds holds every small case at seeds 1 .. 11 of its inputs as well, under the same bounds.  Together the two
tests are the measurement behind the table in classifier_cover's docstring: when the module is done, the `worst` fixture prints the worst fp32
ratio of every ceiling family over whatever ran (`CLASSIFIER-COVER-WORST`; the whole file gives the `measured` column).  It prints and checks
nothing: every bound is asserted where its case runs."""
import pytest
import torch

from tests import classifier_cover as C

pytestmark = pytest.mark.gpu
SMALL_OPS = sorted({c.op for c in C.CASES if not C.is_large(c)})


@pytest.fixture(scope="module")
def K():
    from gansynth_amd import kernels
    return kernels.get()


@pytest.fixture(scope="module")
def worst():
    ratios = {}
    yield ratios
    for family in sorted(ratios):
        measured, suite, here = C.CEILINGS[family]
        print(f"CLASSIFIER-COVER-WORST {family} {ratios[family]:.3e} suite {suite:g} here {here:g}")


def _hold(c, got, ref, worst, seed=0):
    """Every result of a case against its reference entry; the fp32 ratios go to the family's worst."""
    failed = []
    for name, entry in ref.items():
        family, ratio, ok = C.within(got[name], entry)
        print(f"CLASSIFIER-COVER {C.case_id(c)} seed {seed} {name} ratio {ratio:.3e}")
        if family is not None and got[name].dtype != torch.bfloat16:
            worst[family] = max(worst.get(family, 0.0), ratio)
        if not ok:
            failed.append((name, ratio))
    assert not failed, (C.case_id(c), seed, failed)


def _library_geometry(K, c):
    """What the library's own host arithmetic says of the case's shape, held against the restatement the case's facts come from."""
    lib = K.lib
    if c.op.startswith("gn_"):
        n, ch, h, w, G = c.shape
        assert lib.gs_group_norm_workspace_bytes(n, h * w, ch, G) == C.gn_workspace_bytes(n, h * w, ch, G)
        assert lib.gs_group_norm_bwd_workspace_bytes(n, h * w, ch, G) == C.gn_bwd_workspace_bytes(n, h * w, ch, G)
    elif c.op == "conv1x1_bwd_weight":
        ci, co, stride, n, h, w = c.shape
        assert lib.gs_conv1x1_bwd_weight_workspace_bytes(n, h, w, ci, co, stride) == C.conv1x1_wgrad_workspace_bytes(n, h, w, ci, co, stride)
    elif c.op == "stem_wgrad":
        assert lib.gs_resnet_stem_bwd_weight_workspace_bytes(*c.shape) == C.stem_wgrad_workspace_bytes(*c.shape)
    elif c.op == "momentum":
        assert lib.gs_momentum_workspace_bytes(c.shape[0]) == C.momentum_workspace_bytes(c.shape[0])
    f = C.facts(c)
    assert all(f[k] == v for k, v in c.want.items()), (C.case_id(c), c.want, f)


@pytest.mark.parametrize("case", C.CASES, ids=C.case_id)
def test_classifier_kernels_match_float64(K, worst, case):
    c = case
    _library_geometry(K, c)
    d = C.inputs(c)
    ref = C.reference(c, d)
    got = C.run(K, c, d)
    again = C.run(K, c, d)
    torch.cuda.synchronize()
    assert sorted(got) == sorted(again)
    for name in got:
        assert torch.equal(got[name], again[name]), (C.case_id(c), name, "two runs differ")
    _hold(c, got, ref, worst)
    # exact zeros: the pixels a stride-2 data gradient skips
    for name, mask in C.zero_masks(c, d).items():
        assert mask.any() and not bool(got[name].cpu()[mask].any()), (C.case_id(c), name)
    if c.op == "max_pool_bwd" and c.dtype == C.F32:   # the gradient lands where the reference's does, and nowhere else
        assert torch.equal(got["gx"].cpu() != 0, ref["gx"].ref != 0)
    if c.op == "stem_pool" and c.args["want_pool"]:   # the fused pool is the max pool of the kernel's own stem, bit for bit -- and the standalone kernel's
        stem = got["stem"].cpu()
        assert torch.equal(got["pool"].cpu(), C.RR.max_pool(stem.float()).to(stem.dtype))
        assert torch.equal(K.max_pool2d(got["stem"]), got["pool"])
    if c.op == "weight_std":
        for i in range(len(c.shape)):
            assert torch.equal(got[f"out{i}"], got[f"single{i}"]), c.shape[i]      # the batched launch: the bits of the per-weight one
            assert not bool(got[f"gout{i}"].any()), c.shape[i]                     # cleared behind the read
            if C._fan(c.shape[i]) == 1:                                            # variance 0: everything is exactly zero
                assert not bool(got[f"out{i}"].any()) and not bool(got[f"gw{i}"].any())
    if c.op == "softmax_xent" and not c.args["want_grad"]:   # the same loss and count as with the gradient
        loss, _, correct = K.softmax_xent(C._dev(d["logits"]), C._dev(d["labels"]), want_grad=True)
        assert torch.equal(loss, got["loss"]) and torch.equal(correct, got["correct"])


@pytest.mark.parametrize("op", SMALL_OPS)
def test_small_cases_at_the_other_seeds(K, worst, op):
    """The small cases of an operation at seeds 1 .. 11 of their inputs, under the bounds of seed 0."""
    n = 0
    for c in C.CASES:
        if c.op != op or C.is_large(c):
            continue
        for seed in C.SEEDS[1:]:
            d = C.inputs(c, seed)
            _hold(c, C.run(K, c, d), C.reference(c, d), worst, seed)
            n += 1
    assert n > 0
