"""GPU: every VALU conv kernel of csrc/conv_thin.hip -- the 1x1 colour convs (thin_expand, thin_reduce, thin_expand_pnbwd), the one-output-channel
kernels (thin_single3, thin_single) and the generic conv_direct -- against float64 on the operands as stored (tests/thin_cover.py: reference), at
an element-wise bound (below).

One test per kernel family, dtype and conv mode; its cases (thin_cover.CASES) reach, between them, every instantiation an entry point can reach.
Every case first asks the library which kernel it runs (gs_conv_thin_route) and asserts that it is the case's own, so no case passes on a
neighbouring kernel; then it prints `THIN-COVER <case> ratio ...` and asserts (run with -s).  The EXPAND and REDUCE cases run twice: here, at the
default grid caps (many blocks, one pass each), and in ONE child process with GS_THIN_EXPAND_BLOCKS = GS_THIN_REDUCE_BLOCKS = 2, where two blocks
make full four-pass trips and tail passes over a ragged pixel count -- the trip loop of thin_expand_kernel and the LC == 4 finishing path of
thin_reduce_kernel.  The child runs its cases one after another under a time limit and is started once, by the first test that needs it.  The bf16
leaky-relu EXPAND cases of 32 k channels also run in their sign-bit form (check_one_bit_leaky_relu_masks: values bit-identical, words correct).

Every element of every result is held to the bound of tests/cover_bounds.py (thin_cover.bound), at seeds 0 .. 11 of the case's operands -- no
longer to the max-norm ceilings (1e-3 fp32, 1e-2 bf16), which the bound is never above.  A bf16 result is rounded once, twice where the route
leaves a pass behind the kernel (a mask; bias and activation ride in every kernel).  The worst ratios measured on the MI355X over the 4584
comparisons of this file are in thin_cover's docstring; the `worst` fixture prints that column when the module is done (THIN-COVER-WORST)."""
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
from tests import thin_cover as C  # noqa: E402

pytestmark = pytest.mark.gpu
KNOBS = ("GS_THIN_EXPAND_BLOCKS", "GS_THIN_REDUCE_BLOCKS")
FAMILIES = C.families()


def check_case(K, c, capped, worst):
    """Route, result (at every seed of the measurement) and, where the case has one, sign-bit form of one case under this process's caps;
    returns the worst error ratio."""
    r = C.route(K.lib, c)
    assert C.route_key(r, c.key.dtype) == c.key, (C.case_id(c), r)
    if c.key.kernel in (C.EXPAND, C.REDUCE):
        assert (r.grid == 2 and r.trips >= 1 and r.tails >= 1) if capped else (r.grid > 2 and (r.trips, r.tails) == (0, 1)), (C.case_id(c), r)
    ratio = 0.0
    for seed in B.seeds_for(C.macs(c)):
        d = C.inputs(c, seed=5 + B.SEED_STRIDE * seed)
        ref, mag = C.reference(c, d), C.mag(c, d)
        m = B.hold("THIN-COVER", f"{C.case_id(c)} {'capped' if capped else 'default'} seed {seed}", C.run(K, c, d), ref, C.bound(c, r, ref, mag), mag,
                   worst, C.family(c))
        ratio = max(ratio, m.ratio)
    if C.bits_case(c):
        from tests.test_kernels_gpu import check_one_bit_leaky_relu_masks
        assert C.route(K.lib, c, want_bits=True).bits_fused == 1, C.case_id(c)
        check_one_bit_leaky_relu_masks(K, (c.n, c.ci, c.co, c.h, c.w, 1, 1), reader_channels=(32,), readers=())
    return ratio


@pytest.fixture(scope="module")
def worst():
    """The measurement behind the table of thin_cover's docstring: printed when the module is done, over whatever ran.  It checks nothing."""
    w = B.Worst()
    yield w
    w.report("THIN-COVER", C.CEILINGS)


@pytest.fixture(scope="module")
def K():
    from gansynth_amd import kernels
    assert not any(k in os.environ for k in KNOBS), "the parent process runs the default grid caps"
    return kernels.HipKernels()


class _CappedChild(object):
    """Every EXPAND and REDUCE case under grid caps of 2, in one child process started when the first test asks; a time limit, no second try."""
    def __init__(self):
        self.results, self.failed = None, None

    def get(self, c):
        if self.results is None and self.failed is None:
            self.failed = ("not finished", "", "")   # (marked before the spawn: whatever happens below, the child is started once)
            env = dict(os.environ, GS_THIN_EXPAND_BLOCKS=str(C.CAPPED[0]), GS_THIN_REDUCE_BLOCKS=str(C.CAPPED[1]))
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
        assert self.failed is None, f"the capped child ended with {self.failed[0]}; it is not started again: {self.failed[1:]}"
        return self.results[C.case_id(c)]

    def take_rows(self):
        """The child's worst rows, once."""
        rows, self.rows = getattr(self, "rows", {}), {}
        return rows


@pytest.fixture(scope="module")
def capped_child():
    return _CappedChild()


@pytest.mark.parametrize("family", sorted(FAMILIES), ids=C.family_id)
def test_thin_kernels_match_float64(K, capped_child, worst, family):
    for c in FAMILIES[family]:
        check_case(K, c, capped=False, worst=worst)
    if family[0] in (C.EXPAND, C.REDUCE):
        for c in FAMILIES[family]:
            res = capped_child.get(c)
            worst.merge(capped_child.take_rows())
            assert res["ok"], (C.case_id(c), res["error"])


def _child():
    """Under the caps of this process's environment: every EXPAND and REDUCE case, checked; one JSON line of results.  A failed assertion is a
    result; anything else (a HIP error among them) ends the child with a non-zero status."""
    from gansynth_amd import kernels
    K, worst = kernels.HipKernels(), B.Worst()
    out = {}
    for c in C.CASES:
        if c.key.kernel not in (C.EXPAND, C.REDUCE):
            continue
        try:
            out[C.case_id(c)] = {"ok": True, "ratio": check_case(K, c, capped=True, worst=worst)}
        except AssertionError as e:
            out[C.case_id(c)] = {"ok": False, "error": str(e)[-1500:]}
    torch.cuda.synchronize()
    out["rows"] = worst.rows
    print(json.dumps(out))


if __name__ == "__main__":
    _child()
