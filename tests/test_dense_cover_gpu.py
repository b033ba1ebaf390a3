"""GPU: every dense kernel of csrc/dense.hip -- forward (generic, small, fast, MFMA, the finalize pass), data gradient (generic, wide, fast, MFMA)
and weight gradient (generic, fast) -- against float64 on the operands as stored (tests/dense_cover.py: reference), at the dense tests' own
ceilings of max |ref|: forward and data gradient 1e-3 fp32 and 2e-2 bf16, weight gradient 1e-3 in both.

One test per kernel template and dtype; its cases (dense_cover.CASES) reach, between them, all 36 compiled instantiations.  Every case first asks
the library which kernel it runs (gs_dense_route) and asserts that it is the case's own instantiation and the path the case is there for (the
slices its finalize pass folds), so no case passes on a neighbouring kernel; then it prints `DENSE-COVER <case> ratio ...` and asserts (run with
-s).  The library reads GS_NO_DENSE_MFMA once per process: the cases that carry the knob -- every MFMA shape once more on the kernels that take
it then -- run in ONE child process, started once under a time limit by the first test that needs it and never a second time.

Every element of every result is held to the bound of tests/cover_bounds.py (dense_cover.bound), at seeds 0 .. 11 of the case's operands -- no
longer to the max-norm ceilings above, which the bound is never above.  The worst ratios measured on the MI355X over the 1536 comparisons of this
file are in dense_cover's docstring; the `worst` fixture prints that column when the module is done (DENSE-COVER-WORST).
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
from tests import cover_bounds as B  # noqa: E402
from tests import dense_cover as C  # noqa: E402

pytestmark = pytest.mark.gpu
KNOB = "GS_NO_DENSE_MFMA"
FAMILIES = C.families()


def check_case(K, c, worst):
    """Route and result (at every seed of the measurement) of one case under this process's knob; returns the worst error ratio."""
    r = C.route(K.lib, c, no_mfma=-1)
    assert not isinstance(r, int) and C.route_key(r, c.key.dtype) == c.key, (C.case_id(c), r)
    assert (r.finalize, r.ksplit if r.finalize else 0) == (int(c.fin > 0), c.fin), (C.case_id(c), r)
    ratio = 0.0
    for seed in B.seeds_for(C.macs(c)):
        d = C.inputs(c, seed=5 + B.SEED_STRIDE * seed)
        ref, mag = C.reference(c, d), C.mag(c, d)
        m = B.hold("DENSE-COVER", f"{C.case_id(c)} seed {seed}", C.run(K, c, d), ref, C.bound(c, ref, mag), mag, worst, C.family(c))
        ratio = max(ratio, m.ratio)
    return ratio


@pytest.fixture(scope="module")
def worst():
    """The measurement behind the table of dense_cover's docstring: printed when the module is done, over whatever ran.  It checks nothing."""
    w = B.Worst()
    yield w
    w.report("DENSE-COVER", C.CEILINGS)


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
                print(r.stdout[-2000000:])
                try:
                    assert r.returncode == 0
                    self.results, self.failed = json.loads(r.stdout.strip().splitlines()[-1]), None
                    self.rows = self.results.pop("rows")
                except (AssertionError, ValueError, IndexError):
                    self.failed = (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
        assert self.failed is None, f"the knob child ended with {self.failed[0]}; it is not started again: {self.failed[1:]}"
        return self.results[C.case_id(c)]

    def take_rows(self):
        """The child's worst rows, once."""
        rows, self.rows = getattr(self, "rows", {}), {}
        return rows


@pytest.fixture(scope="module")
def knob_child():
    return _KnobChild()


@pytest.mark.parametrize("family", sorted(FAMILIES), ids=C.family_id)
def test_dense_kernels_match_float64(K, knob_child, worst, family):
    for c in FAMILIES[family]:
        if not c.no_mfma:
            check_case(K, c, worst)
    for c in FAMILIES[family]:
        if c.no_mfma:
            res = knob_child.get(c)
            worst.merge(knob_child.take_rows())
            assert res["ok"], (C.case_id(c), res["error"])


def _child():
    """With the knob of this process's environment: every case that carries it, checked; one JSON line of results.  A failed assertion is a
    result; anything else (a HIP error among them) ends the child with a non-zero status."""
    from gansynth_amd import kernels
    K, worst = kernels.HipKernels(), B.Worst()
    out = {}
    for c in C.CASES:
        if not c.no_mfma:
            continue
        try:
            out[C.case_id(c)] = {"ok": True, "ratio": check_case(K, c, worst)}
        except AssertionError as e:
            out[C.case_id(c)] = {"ok": False, "error": str(e)[-1500:]}
    torch.cuda.synchronize()
    out["rows"] = worst.rows
    print(json.dumps(out))


if __name__ == "__main__":
    _child()
