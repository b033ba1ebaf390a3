"""GPU: every compiled implicit-GEMM conv kernel -- each (mode, dtype, configuration) of conv_igemm.hip's table (gs_conv_igemm_table) -- computes
its convolution, element by element against a float64 reference (tests/igemm_cover.py: conv_ref64).

One test per kernel.  Its shapes are the cheapest ones, and the cheapest ragged ones, that the chooser routes to that kernel ON THIS DEVICE
(igemm_cover.find_shapes), and every test first asserts that gs_conv_igemm_config still answers the kernel's own row for them, so no test passes on
a neighbouring kernel.  Plain rows run through both entry points of their mode (their weight preparation differs); the fused-norm rows run the
assertions of the three fused-norm tests of tests/test_kernels_gpu.py at their shapes; the bf16 plain rows also run in their sign-bit form
(test_one_bit_leaky_relu_masks' assertions: bit-identical to the values path).  Kernels only a measurement knob of the chooser reaches run in a
fresh child process per knob setting (the knobs are read once), one after another.

The plain rows are held element by element to the bound of tests/cover_bounds.py (igemm_cover.plain_bound: (K + 3) 2^-24 of the element's own
magnitude, capped by the ceiling of igemm_cover.CEILINGS, plus the one bf16 rounding of a bf16 result), at seeds 0 .. 11 of every case of at most
5e7 multiply-adds and at seed 0 of the others; every comparison prints its max-norm ratio and its worst err / bound before it asserts (run with
-s), and when the module is done the `worst` fixture prints the column behind the table of igemm_cover's docstring (IGEMM-COVER-WORST), where
the measured ratios are recorded."""
import json
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tests import cover_bounds as B  # noqa: E402
from tests import igemm_cover as C  # noqa: E402

pytestmark = pytest.mark.gpu
TORCH_DTYPE = {C.F32: torch.float32, C.BF16: torch.bfloat16}


def _kernels():
    from gansynth_amd import _lib
    return C.table(_lib.load())   # (host only: collecting this file needs no device)


def _dev(t, dtype=torch.float32):
    t = t.to("cuda", dtype)
    return t.contiguous(memory_format=torch.channels_last) if t.dim() == 4 else t


def _run_plain(K, call, a, wt, alpha, s):
    n, h, w, ci, co = C.layer_args(call, *s[:5])
    conv = () if call.transposed else (3, call.stride)   # (the transposed methods take no kernel size and stride)
    if call.data_grad and not call.transposed:
        return K.conv2d_bwd_data(a, wt, (n, ci, h, w), *conv, alpha)
    return getattr(K, call.name)(a, wt, *conv, alpha)


def check_kernel(K, E, kernel, shapes, worst):
    """All assertions for one kernel at its shapes; returns the worst plain error ratio (None for a fused-norm row) and notes every plain
    comparison in `worst` (cover_bounds.Worst)."""
    from tests.test_kernels_gpu import (check_conv_bias_act_norm, check_data_gradient_through_pixel_norm, check_one_bit_leaky_relu_masks,
                                        check_second_order_norm_gradients)
    dtype, norm = TORCH_DTYPE[kernel.dtype], kernel.cfg[6]
    top = None
    for s in shapes:
        assert C.config(K.lib, kernel.mode, kernel.dtype, s) == (kernel.cfg, 1), (C.kernel_id(kernel), s, C.config(K.lib, kernel.mode, kernel.dtype, s))
        kind = "conv" if kernel.mode == C.S1 else "convT"
        if norm == C.PLAIN:
            family = f"plain-{C.DTYPE_NAMES[kernel.dtype]}"
            for second in (False, True):
                call = C.api_call(kernel.mode, C.PLAIN, second)
                for seed in B.seeds_for(C.macs(kernel.mode, s)):
                    a, wt, alpha = C.plain_inputs(call, s, seed=17 + second + B.SEED_STRIDE * seed)
                    bf16 = kernel.dtype == C.BF16
                    ref, mag = C.conv_ref64(call, a, wt, alpha, bf16=bf16), C.conv_mag(call, a, wt, alpha, bf16=bf16)
                    got = _run_plain(K, call, _dev(a, dtype), _dev(wt), alpha, s)
                    m = B.hold("IGEMM-COVER", f"{C.kernel_id(kernel)} {call.name} {tuple(s)} seed {seed}", got, ref, C.plain_bound(kernel, s, ref, mag),
                               mag, worst, family)
                    top = m.ratio if top is None else max(top, m.ratio)
        elif norm == C.NORM_FWD:       # S1: the stride-1 conv, T2: the transposed conv -- (kind, n, ci, co, h, w)
            assert kernel.mode in (C.S1, C.T2)
            check_conv_bias_act_norm(K, E, (kind, s.n, s.ic, s.oc, s.hb, s.wb), dtype)
        elif norm == C.NORM_BWD:       # S1: the stride-1 conv's data gradient, S2: the transposed conv's -- ci: the channels of gx, the kernel's oc
            assert kernel.mode in (C.S1, C.S2)
            for with_addend in (False, True):
                check_data_gradient_through_pixel_norm(K, E, (kind, s.n, s.oc, s.ic, s.hb, s.wb), dtype, with_addend)
        else:
            assert kernel.mode in (C.S1, C.T2)
            check_second_order_norm_gradients(K, E, (kind, s.n, s.ic, s.oc, s.hb, s.wb), dtype)
        if norm == C.PLAIN and kernel.dtype == C.BF16:
            # the sign-bit form of this kernel at this shape: S1 / S2 write the words (forward with leaky relu) and read them (masked launches with
            # ic channels on the other side: the same kernel-role shape); T2 reads the words of a stride-1 result on its fine grid
            if kernel.mode == C.T2:
                check_one_bit_leaky_relu_masks(K, (s.n, 32, s.oc, 2 * s.hb, 2 * s.wb, 3, 1), reader_channels=(s.ic,), readers=("bwd_data_s2",))
            elif kernel.mode == C.S1:
                check_one_bit_leaky_relu_masks(K, (s.n, s.ic, s.oc, s.hb, s.wb, 3, 1), reader_channels=(s.ic,), readers=("bwd_data", "fwd_mask"))
            else:
                check_one_bit_leaky_relu_masks(K, (s.n, s.ic, s.oc, 2 * s.hb, 2 * s.wb, 3, 2), reader_channels=(s.ic,), readers=("fwd_mask_s2",))
    return top


@pytest.fixture(scope="module")
def K():
    from gansynth_amd import kernels
    return kernels.HipKernels()


@pytest.fixture(scope="module")
def E():
    from tests.cpu_kernels import CpuEmuKernels
    return CpuEmuKernels()


@pytest.fixture(scope="module")
def worst():
    """The measurement behind the table of igemm_cover's docstring: printed when the module is done, over whatever ran.  It checks nothing:
    every bound is asserted where its case runs."""
    w = B.Worst()
    yield w
    w.report("IGEMM-COVER", C.CEILINGS)


@pytest.fixture(scope="module")
def default_shapes(K):
    assert not any(k in os.environ for k in C.KNOBS), "the parent process runs the default knobs"
    return C.find_shapes(K.lib)


class _KnobChildren(object):
    """The kernels the default knobs do not reach, run by one child process per knob setting -- started when the first such kernel's test asks,
    one after another, each with a time limit; after a child that did not end cleanly no further child starts."""
    def __init__(self, wanted):
        self.wanted, self.results, self.failed = [C.kernel_id(k) for k in wanted], None, None

    def get(self, kernel):
        if self.results is None:
            self.results = {}
            left = list(self.wanted)
            env = {k: v for k, v in os.environ.items() if k not in C.KNOBS}
            env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
            for knobs in C.KNOB_SETTINGS[1:]:
                if not left:
                    break
                r = subprocess.run([sys.executable, os.path.abspath(__file__), json.dumps(left)], env={**env, **knobs}, capture_output=True, text=True, timeout=600)
                print(r.stdout[-200000:])
                if r.returncode != 0:
                    self.failed = (knobs, r.returncode, r.stdout[-1500:], r.stderr[-3000:])
                    break
                done = json.loads(r.stdout.strip().splitlines()[-1])
                self.results.update({k: dict(v, knobs=knobs) for k, v in done.items()})
                left = [k for k in left if k not in done]
        assert self.failed is None, f"the child under {self.failed[0]} ended with {self.failed[1]}; no further child was started: {self.failed[2:]}"
        return self.results.get(C.kernel_id(kernel))


@pytest.fixture(scope="module")
def knob_children(default_shapes):
    return _KnobChildren([k for k in _kernels() if k not in default_shapes])


@pytest.mark.parametrize("kernel", _kernels(), ids=C.kernel_id)
def test_compiled_kernel_computes_its_convolution(K, E, default_shapes, knob_children, worst, kernel):
    if kernel in default_shapes:
        check_kernel(K, E, kernel, default_shapes[kernel], worst)
        return
    res = knob_children.get(kernel)
    assert res is not None, f"{C.kernel_id(kernel)}: no shape of the grid reaches it on this device under any knob setting"
    worst.merge(res["rows"])
    print(f"IGEMM-COVER {C.kernel_id(kernel)} under {res['knobs']}: {res}")
    assert res["ok"], res["error"]


def _child(wanted):
    """Under the knobs of this process's environment: every wanted kernel the grid reaches here, checked; one JSON line of results.  A failed
    assertion is a result; anything else (a HIP error among them) ends the child with a non-zero status."""
    from gansynth_amd import kernels
    from tests.cpu_kernels import CpuEmuKernels
    K, E = kernels.HipKernels(), CpuEmuKernels()
    found = C.find_shapes(K.lib)
    out = {}
    for k, shapes in found.items():
        if C.kernel_id(k) not in wanted:
            continue
        worst = B.Worst()
        try:
            out[C.kernel_id(k)] = {"ok": True, "worst": check_kernel(K, E, k, shapes, worst), "shapes": [list(s) for s in shapes]}
        except AssertionError as e:
            out[C.kernel_id(k)] = {"ok": False, "error": str(e)[-1500:], "shapes": [list(s) for s in shapes]}
        out[C.kernel_id(k)]["rows"] = worst.rows
    torch.cuda.synchronize()
    print(json.dumps(out))


if __name__ == "__main__":
    _child(set(json.loads(sys.argv[1])))
