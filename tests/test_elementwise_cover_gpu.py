"""GPU: every kernel of csrc/elementwise.hip that the route covers -- bias + activation, the activation gradients, axpby, row scale, upscale and
block sums, the channel sums with their finalize passes, the fused activation-backward sums, pixel norm in all orders with its fused forms and
bias sums, sums of squares per row -- and the three batch-stddev kernels of csrc/small_ops.hip, in fp32 and bf16, against float64 on the operands
as stored (tests/elementwise_cover.py: reference).

One test per kernel template and dtype; its cases (elementwise_cover.CASES) reach, between them, all 86 compiled instantiations and every path
inside them.  Every case first asks the library which kernel it runs (gs_elementwise_route, caps -1) and asserts that it is the case's own
instantiation and the path the case is there for, so no case passes on a neighbouring kernel; then it prints `ELEMENTWISE-COVER <case> ratio ...`
and asserts (run with -s).  The library reads GS_EW_GRID_CAP and GS_PN_BIAS_GRID_CAP once per process: every case runs a second time with both
set to 2 -- two blocks, so that every grid-stride loop takes several trips at these small shapes -- in ONE child process, started once under a time
limit by the first test that needs it and never a second time.

Ceilings (max error over max |ref|, igemm_cover.ratio) for fp32 results, the fp32 sums of bf16 inputs among them: 1e-5 forward, streaming and sums;
1e-4 first- and second-order norm and stddev gradients; 1e-6 axpby and row_scale.  A bf16 result is computed in fp32 and rounded once to nearest
even: element by element |got - ref| <= 2^-8 |ref| + ceiling * max |ref|.  Upscale at scale 1 is bit-exact.

Worst ratios measured on the MI355X over the 1190 comparisons of this file, knobs unset / set to 2 (fp32 results, then the fp32 sums the bf16 cases
leave; bf16 results in brackets: their bound is the element-wise one, and every one of them held it):
  bias_act 6.6e-8 / 6.6e-8 [2.5e-3 / 2.5e-3];  bias_act_scalar 8.8e-8 / 8.8e-8 [2.0e-3 / 2.0e-3];  act_bwd 2.8e-7 / 2.8e-7 [3.5e-3 / 3.5e-3];
  tanh_bwd_bwd 6.7e-8 / 6.7e-8 [2.5e-3 / 2.5e-3];  axpby and axpby_dev 6.4e-8 / 6.4e-8 [3.1e-3 / 3.1e-3];  upscale 0 / 0 [0 / 0];
  row_scale 3.8e-8 / 3.8e-8 [2.4e-3 / 2.4e-3];  channel_sum 2.8e-7 / 2.8e-7, of bf16 3.3e-7 / 3.3e-7;  channel_sum_rows 2.3e-7 / 2.3e-7, of bf16
  9.2e-8 / 9.2e-8;  act_bwd_sum 4.5e-7 / 4.5e-7, of bf16 5.7e-7 / 5.7e-7 [2.4e-3 / 2.4e-3];  pixel_norm (all orders, every fused form) 2.8e-7 / 2.8e-7,
  bias sums of bf16 1.4e-7 / 1.8e-7 [3.2e-3 / 3.2e-3];  blocksum 1.7e-7 / 1.7e-7 [3.3e-3 / 3.3e-3];  blocksum_small 7.5e-8 / 7.5e-8 [2.9e-3 / 2.9e-3];
  sumsq_rows 4.5e-8 / 4.5e-8, of bf16 7.1e-8 / 7.1e-8;  batch_stddev_fwd 1.2e-7 / 1.2e-7 [2.4e-3 / 2.4e-3];  batch_stddev_bwd 8.6e-7 / 8.6e-7
  [3.6e-3 / 3.6e-3];  batch_stddev_bwd_bwd 1.1e-6 / 1.1e-6 [2.7e-3 / 2.7e-3].
The first run of this file found the bias sums of the two-pass gs_act_bwd_bias (c % 4 != 0, c > 1024, 256 % (c/4) != 0) taken over the STORED gradient:
in bf16 1.2e-4 .. 3.8e-3 of the largest sum away from the float64 sums (cases act_bwd_bias-bf16 77x2, 77x12, 77x61), where the one-pass kernel, which
sums its values before it rounds them, is at 5.7e-7.  The second pass now sums g * act'(y) as computed.
"""
import json
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tests import elementwise_cover as C  # noqa: E402

pytestmark = pytest.mark.gpu
FAMILIES = C.families()


def check_case(K, c, knobs):
    """Route and results of one case under this process's knobs; returns {result name: error ratio}."""
    r = C.route(K.lib, c)
    assert not isinstance(r, int) and c.key in C.route_keys(c.op, c.dtype, r, c.args), (C.case_id(c), r)
    f = C.facts(c, r)
    assert all(f[k] == v for k, v in c.want.items() if knobs is None or k not in ("trips", "grid_x")), (C.case_id(c), c.want, f)
    assert r == C.route(K.lib, c, *((C.EW_CAP, C.PN_BIAS_CAP) if knobs is None else knobs)), (C.case_id(c), r)   # the caps this process reads
    d = C.inputs(c)
    got, ref = C.run(K, c, d), C.reference(c, d)
    assert set(got) == set(ref)
    ratios, bad = {}, []
    for name in sorted(ref):
        ratios[name], ok = C.within(c, name, got[name], ref[name])
        print(f"ELEMENTWISE-COVER {C.case_id(c)} {name} {str(got[name].dtype)[6:]} ratio {ratios[name]:.3e}")
        if not ok:
            bad.append(name)
    assert not bad, (C.case_id(c), bad, ratios)
    return ratios


@pytest.fixture(scope="module")
def K():
    from gansynth_amd import kernels
    assert not set(C.KNOBS) & set(os.environ), "the parent process runs with both knobs unset"
    return kernels.HipKernels()


class _KnobChild(object):
    """Every case once more with the knobs set, in one child process started when the first test asks; a time limit, no second try."""
    def __init__(self):
        self.results, self.failed = None, None

    def get(self, c):
        if self.results is None and self.failed is None:
            self.failed = ("not finished", "", "")   # (marked before the spawn: whatever happens below, the child is started once)
            env = dict(os.environ, **C.KNOBS)
            env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
            try:
                r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=300)
            except subprocess.TimeoutExpired as e:
                self.failed = ("the time limit", str(e.stdout)[-1500:], str(e.stderr)[-3000:])
            else:
                print(r.stdout[-200000:])
                try:
                    assert r.returncode == 0
                    self.results, self.failed = json.loads(r.stdout.strip().splitlines()[-1]), None
                except (AssertionError, ValueError, IndexError):
                    self.failed = (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
        assert self.failed is None, f"the knob child ended with {self.failed[0]}; it is not started again: {self.failed[1:]}"
        return self.results[C.case_id(c)]


@pytest.fixture(scope="module")
def knob_child():
    return _KnobChild()


@pytest.mark.parametrize("family", sorted(FAMILIES), ids=C.family_id)
def test_elementwise_kernels_match_float64(K, knob_child, family):
    for c in FAMILIES[family]:
        check_case(K, c, None)
    for c in FAMILIES[family]:
        res = knob_child.get(c)
        assert res["ok"], (C.case_id(c), res["error"])


def _child():
    """With the knobs of this process's environment: every case, checked; one JSON line of results.  A failed assertion is a result; anything
    else (a HIP error among them) ends the child with a non-zero status."""
    from gansynth_amd import kernels
    knobs = tuple(int(os.environ[k]) for k in ("GS_EW_GRID_CAP", "GS_PN_BIAS_GRID_CAP"))
    K = kernels.HipKernels()
    out = {}
    for c in C.CASES:
        try:
            out[C.case_id(c)] = {"ok": True, "ratio": check_case(K, c, knobs)}
        except AssertionError as e:
            out[C.case_id(c)] = {"ok": False, "error": str(e)[-1500:]}
    torch.cuda.synchronize()
    print(json.dumps(out))


if __name__ == "__main__":
    _child()
