"""CPU: the cases of tests/test_igemm_cover_gpu.py exist and mean something (no GPU: the chooser answers for the MI355X's 256 CUs).

Reachability: every (mode, dtype, configuration) of the table of compiled implicit-GEMM kernels (gs_conv_igemm_table) is what the chooser
(gs_conv_igemm_config) answers for some shape of tests/igemm_cover.py's grid, under the default knobs or, failing that, under one of the
chooser's measurement knobs.  A kernel nothing reaches is dead code or a gap of the grid.  Every chosen case stays under igemm_cover.MAX_MACS
for its float64 reference.  (The grid holds one output-channel count beyond the layers' own, 352 = 5 * 64 + 32: the two transposed kernels with
A = 1, TG = 3 run only layers whose channel count is no multiple of 64 and that have more blocks than the chip has CUs, counted in whole
64-channel tiles -- with 96 channels that takes 64 images of 32 rows, 2.5e9 to 5.4e9 multiply-adds in bf16.)

Sensitivity: the GPU test's tolerance is not vacuous -- a result that lost ONE (tap, 32-channel chunk) stage of the K loop differs from the
reference by at least ten times that tolerance, at every plain case small enough to evaluate twice here."""
import pytest
import torch

from tests import cover_bounds as B
from tests import igemm_cover as C


@pytest.fixture(scope="module")
def lib():
    from gansynth_amd import _lib
    assert (C.F32, C.BF16) == (_lib.GS_F32, _lib.GS_BF16)
    return _lib.load()


@pytest.fixture(scope="module")
def plan():
    return C.assignment()


def test_table_is_the_compiled_rows(lib):
    import ctypes
    rows, out = C.rows(lib), (ctypes.c_int * 11)()
    assert len(rows) == 43 and len(C.table(lib)) == 77 == len(set(C.table(lib)))
    assert sum(1 for k in C.table(lib) if k.dtype == C.BF16 and k.cfg[6] == C.PLAIN) == 32   # the rows that also have a sign-bit form: 109 symbols
    assert lib.gs_conv_igemm_table(len(rows), out) == -1 and lib.gs_conv_igemm_table(-1, out) == -1 and lib.gs_conv_igemm_table(0, None) == -1
    for r in rows:
        assert r[0] in (C.S1, C.S2, C.T2) and r[1] in (0, 1) and r[6] in (0, 1) and r[8] in range(4) and r[10] in (0, 1), r
    cfg_out = (ctypes.c_int * 10)()   # the chooser's answer for the top-of-pyramid layer is a row of the table, spelled the same way
    assert lib.gs_conv_igemm_config(C.S1, 8, 128, 1024, 32, 32, C.BF16, C.NORM_FWD, cfg_out) == 0 and cfg_out[9] == 1
    assert C.Kernel(C.S1, C.BF16, tuple(cfg_out[:9])) in C.table(lib)


def test_every_compiled_kernel_is_reached_by_a_case_under_the_cap(lib, plan):
    reached = {}
    for knobs, found in plan:
        for k, shapes in found.items():
            assert k not in reached
            reached[k] = (knobs, shapes)
    missing = [C.kernel_id(k) for k in C.table(lib) if k not in reached]
    assert not missing, f"compiled, but no shape of the grid runs them under any knob setting: {missing}"
    assert set(reached) == set(C.table(lib)), [C.kernel_id(k) for k in reached if k not in C.table(lib)]
    total = 0
    for k, (knobs, shapes) in reached.items():
        assert 1 <= len(shapes) <= 2
        for s in shapes:
            assert s.want == k.cfg[6] and C.api_call(k.mode, s.want) is not None
            assert C.macs(k.mode, s) <= C.MAX_MACS, (C.kernel_id(k), s, C.macs(k.mode, s))
            total += C.macs(k.mode, s) * (2 if s.want == C.PLAIN else 1)
        assert C.raggedness(k, shapes[-1]) >= 1, (C.kernel_id(k), shapes)   # every kernel has a case with a partial tile
    print(f"{len(reached)} kernels, {sum(len(v[1]) for v in reached.values())} shapes, {total:.3g} reference multiply-adds; "
          f"by knob setting: {[(knobs, len(found)) for knobs, found in plan]}")


def test_default_process_finds_what_its_child_found(lib, plan):
    """find_shapes is a function of the knobs alone: this process (default knobs) and the default child agree, shape for shape."""
    import os
    assert not any(k in os.environ for k in C.KNOBS), "the cases are searched under the default knobs"
    assert C.find_shapes(lib) == {k: v for k, v in plan[0][1].items()}


@pytest.mark.parametrize("mode,second", [(m, s) for m in (C.S1, C.S2, C.T2) for s in (False, True)])
def test_reference_agrees_with_the_cpu_emulation(mode, second):
    """conv_ref64 (torch's own conv / conv_transpose in float64) against tests/cpu_kernels.py (autograd of the oracle's convs, fp32): the three
    maps and their data gradients at one small ragged shape each."""
    from tests.cpu_kernels import CpuEmuKernels
    E = CpuEmuKernels()
    call = C.api_call(mode, C.PLAIN, second)
    s = C.Shape(2, 3, 5, 32, 64, C.PLAIN)
    a, wt, alpha = C.plain_inputs(call, s, seed=1)
    n, h, w, ci, co = C.layer_args(call, *s[:5])
    conv = () if call.transposed else (3, call.stride)
    emu = E.conv2d_bwd_data(a, wt, (n, ci, h, w), *conv, alpha) if (call.data_grad and not call.transposed) else getattr(E, call.name)(a, wt, *conv, alpha)
    ref = C.conv_ref64(call, a, wt, alpha)
    assert tuple(ref.shape) == tuple(emu.shape) and ref.dtype == torch.float64
    assert C.ratio(emu, ref) <= 1e-5   # fp32 accumulation of 9 * 32 resp. 9 * 64 terms
    rounded = C.conv_ref64(call, a, wt, alpha, bf16=True)   # the bf16 reference is the same map on rounded operands: within 2 * 2^-9 per product
    assert 1e-5 < C.ratio(rounded, ref) < 2e-2


def test_a_dropped_stage_is_ten_tolerances_away(plan):
    """One (tap, 32-channel chunk) of the weight zeroed in the reference moves the result by >= 10 x the GPU test's tolerance for the shape and
    dtype (same measure: max error over max |ref|), for both entry points of every plain case of at most 5e7 multiply-adds."""
    checked, worst = 0, {}
    for knobs, found in plan:
        for k, shapes in found.items():
            for s in shapes:
                if s.want != C.PLAIN or C.macs(k.mode, s) > 5e7:
                    continue
                for second in (False, True):
                    call = C.api_call(k.mode, C.PLAIN, second)
                    a, wt, alpha = C.plain_inputs(call, s, seed=3)
                    bf16 = k.dtype == C.BF16
                    ref = C.conv_ref64(call, a, wt, alpha, bf16=bf16)
                    for drop in ((0, (s.ic - 1) // 32), (4, 0)):   # a corner tap's last chunk, the centre tap's first
                        moved = C.ratio(C.conv_ref64(call, a, wt, alpha, bf16=bf16, drop=drop), ref)
                        worst[k.dtype] = min(worst.get(k.dtype, moved), moved)
                        assert moved >= 10 * C.TOLERANCE[k.dtype], (C.kernel_id(k), s, call.name, drop, moved)
                        checked += 1
    print(f"{checked} dropped stages, the least visible per dtype (fp32, bf16): {worst}")
    assert checked >= 100 and set(worst) == {C.F32, C.BF16}


# ------------------------------------------------------------------------------------------------ the element-wise bound (tests/cover_bounds.py)
def test_table_is_the_constants_and_the_bound_is_never_weaker():
    """The docstring's table is CEILINGS, every ceiling is what the rule gives for its measurement, and the bound at its largest stays under the
    max-norm tolerance the plain rows were held to before, for both dtypes."""
    B.check_table(C.__doc__, C.CEILINGS)
    for dtype, r in ((C.F32, 0), (C.BF16, 1)):
        for family, (measured, suite, here) in C.CEILINGS.items():
            assert suite == C.TOLERANCE[C.F32] and B.never_weaker(C.TOLERANCE[dtype], here, r), (family, dtype, r)
    assert not B.never_weaker(C.TOLERANCE[C.BF16], 1e-2, 1)   # (the inequality can fail: it is no tautology)
    assert B.U_BF16_MFMA in (2.0 ** -24, 2.0 ** -23)


def _small_plain_cases(plan):
    for knobs, found in plan:
        for k, shapes in found.items():
            for s in shapes:
                if s.want == C.PLAIN and C.macs(k.mode, s) <= B.SMALL_MACS:
                    for second in (False, True):
                        yield k, s, C.api_call(k.mode, C.PLAIN, second)


def test_an_honest_kernel_is_inside_the_bound(plan):
    """The map restated in fp32 on the operands as stored (torch's CPU conv, a bf16 store for the bf16 rows) stays inside the bound at every
    plain case of at most 5e7 multiply-adds, through both entry points."""
    worst, n = {}, 0
    for k, s, call in _small_plain_cases(plan):
        a, wt, alpha = C.plain_inputs(call, s, seed=3)
        bf16 = k.dtype == C.BF16
        ref, mag = C.conv_ref64(call, a, wt, alpha, bf16=bf16), C.conv_mag(call, a, wt, alpha, bf16=bf16)
        m = B.measure(f"{C.kernel_id(k)} {call.name} {tuple(s)}", C.conv_restated(call, a, wt, alpha, bf16=bf16), ref, C.plain_bound(k, s, ref, mag), mag)
        assert m.over == 0 and m.compared == ref.numel() and m.worst <= 1, m.message
        worst[k.dtype] = max(worst.get(k.dtype, 0.0), m.worst)
        n += 1
    print(f"{n} honest results, worst err / bound per dtype (fp32, bf16): {worst}")
    assert n >= 90 and set(worst) == {C.F32, C.BF16}


def _halves(call, wt):
    """The weight with the second resp. the first half of its contracted channels zeroed: two K partials."""
    axis = 3 if call.data_grad else 2
    half = wt.shape[axis] // 2
    lo, hi = wt.clone(), wt.clone()
    lo.narrow(axis, half, wt.shape[axis] - half).zero_()
    hi.narrow(axis, 0, half).zero_()
    return lo, hi


def test_subtly_wrong_kernels_pass_the_old_assertion_and_fail_the_bound(plan):
    """M1 .. M5 of tests/cover_bounds.py's Gap, each built from the float64 reference the way conv_ref64(drop=...) builds the dropped stage:
    M1 (bf16 rows) two K partials each rounded to bf16 before the last add; M2 (bf16 rows) alpha folded into the weight before its bf16
    rounding; M3 (bf16 rows) a truncating store; M4 (fp32 rows) the centre tap's weights rounded to bf16; M5 every element under 5 % of the
    largest scaled by 1 + 2^-6."""
    gap = B.Gap(("M1", "M2", "M3", "M4", "M5"))
    for k, s, call in _small_plain_cases(plan):
        a, wt, alpha = C.plain_inputs(call, s, seed=3)
        bf16 = k.dtype == C.BF16
        ref, mag = C.conv_ref64(call, a, wt, alpha, bf16=bf16), C.conv_mag(call, a, wt, alpha, bf16=bf16)
        bnd, tag, old = C.plain_bound(k, s, ref, mag), f"{C.kernel_id(k)} {call.name} {tuple(s)}", C.TOLERANCE[k.dtype]
        if bf16:
            lo, hi = _halves(call, wt)
            folded = B.fold_through_bf16(C.conv_ref64(call, a, lo, alpha, bf16=True), C.conv_ref64(call, a, hi, alpha, bf16=True))
            gap.check("M1", tag, B.bf16_rne(folded), ref, bnd, old)
            gap.check("M2", tag, B.bf16_rne(C.conv_ref64(call, a.bfloat16(), (alpha * wt).bfloat16(), 1.0)), ref, bnd, old)
            gap.check("M3", tag, B.bf16_truncate(ref), ref, bnd, old)
            gap.check("M5", tag, B.stored_as(B.scale_small(ref), bf16=True), ref, bnd, old)
        else:
            w4 = wt.clone()
            w4[1, 1] = wt[1, 1].bfloat16().float()
            gap.check("M4", tag, C.conv_ref64(call, a, w4, alpha).float(), ref, bnd, old)
            gap.check("M5", tag, B.stored_as(B.scale_small(ref), bf16=False), ref, bnd, old)
    gap.close()
