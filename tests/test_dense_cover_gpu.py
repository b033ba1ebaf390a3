"""GPU: every dense kernel of csrc/dense.hip -- forward (generic, small, fast, MFMA, the finalize pass), data gradient (generic, wide, fast, MFMA)
and weight gradient (generic, fast) -- against float64 on the operands as stored (tests/dense_cover.py: reference), at the dense tests' own
ceilings of max |ref|: forward and data gradient 1e-3 fp32 and 2e-2 bf16, weight gradient 1e-3 in both.

One test per kernel template and dtype; its cases (dense_cover.CASES) reach, between them, all 36 compiled instantiations.  Every case first asks
the library which kernel it runs (gs_dense_route) and asserts that it is the case's own instantiation and the path the case is there for (the
slices its finalize pass folds), so no case passes on a neighbouring kernel; then it prints `DENSE-COVER <case> ratio ...` and asserts (run with
-s).  The library reads GS_NO_DENSE_MFMA once per process: the cases that carry the knob -- every MFMA shape once more on the kernels that take
it then -- run in ONE child process, started once under a time limit by the first test that needs it and never a second time.

Worst ratios measured on the MI355X over the 128 comparisons of this file (max error over max |ref|), knob unset and set together:
  fwd fp32 1.1e-7, bf16 2.7e-3;  fwd_small fp32 2.9e-7, bf16 3.0e-3;  fwd_fast fp32 4.7e-7, bf16 3.2e-3;  fwd_mfma fp32 1.9e-7, bf16 2.4e-3
  (each with the finalize pass where one follows);  bwd_data fp32 1.6e-7, bf16 3.1e-3;  bwd_data_wide fp32 7.6e-8, bf16 1.8e-3;
  bwd_data_fast fp32 9.9e-8, bf16 3.0e-3;  bwd_data_mfma fp32 4.2e-7, bf16 3.1e-3;  bwd_weight fp32 2.1e-7, bf16 6.9e-8;
  bwd_weight_fast fp32 1.1e-7, bf16 8.1e-8
(bf16: the rounding of the result itself, 2^-9 of its size; the weight gradient is fp32 in both).  Every bf16 ratio stays under the conv suite's
1e-2; the ceilings here are the dense tests' 2e-2 all the same.
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
from tests import dense_cover as C  # noqa: E402

pytestmark = pytest.mark.gpu
KNOB = "GS_NO_DENSE_MFMA"
FAMILIES = C.families()


def check_case(K, c):
    """Route and result of one case under this process's knob; returns the error ratio."""
    r = C.route(K.lib, c, no_mfma=-1)
    assert not isinstance(r, int) and C.route_key(r, c.key.dtype) == c.key, (C.case_id(c), r)
    assert (r.finalize, r.ksplit if r.finalize else 0) == (int(c.fin > 0), c.fin), (C.case_id(c), r)
    d = C.inputs(c)
    ratio = C.ratio(C.run(K, c, d), C.reference(c, d))
    print(f"DENSE-COVER {C.case_id(c)} ratio {ratio:.3e}")
    assert ratio <= C.TOLERANCE[c.map][c.key.dtype], (C.case_id(c), ratio)
    return ratio


@pytest.fixture(scope="module")
def K():
    from gansynth_amd import kernels
    assert KNOB not in os.environ, "the parent process runs with the knob unset"
    return kernels.HipKernels()


class _KnobChild(object):
    """Every case that carries the knob, in one child process started when the first test asks; a time limit, no second try."""
    def __init__(self):
        self.results, self.failed = None, None

    def get(self, c):
        if self.results is None and self.failed is None:
            self.failed = ("not finished", "", "")   # (marked before the spawn: whatever happens below, the child is started once)
            env = dict(os.environ, **{KNOB: "1"})
            env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
            try:
                r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=300)
            except subprocess.TimeoutExpired as e:
                self.failed = ("the time limit", str(e.stdout)[-1500:], str(e.stderr)[-3000:])
            else:
                print(r.stdout[-20000:])
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
def test_dense_kernels_match_float64(K, knob_child, family):
    for c in FAMILIES[family]:
        if not c.no_mfma:
            check_case(K, c)
    for c in FAMILIES[family]:
        if c.no_mfma:
            res = knob_child.get(c)
            assert res["ok"], (C.case_id(c), res["error"])


def _child():
    """With the knob of this process's environment: every case that carries it, checked; one JSON line of results.  A failed assertion is a
    result; anything else (a HIP error among them) ends the child with a non-zero status."""
    from gansynth_amd import kernels
    K = kernels.HipKernels()
    out = {}
    for c in C.CASES:
        if not c.no_mfma:
            continue
        try:
            out[C.case_id(c)] = {"ok": True, "ratio": check_case(K, c)}
        except AssertionError as e:
            out[C.case_id(c)] = {"ok": False, "error": str(e)[-1500:]}
    torch.cuda.synchronize()
    print(json.dumps(out))


if __name__ == "__main__":
    _child()
