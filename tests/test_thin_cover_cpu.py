"""CPU: the cases of tests/test_thin_cover_gpu.py exist and mean something (no GPU: gs_conv_thin_route is host arithmetic on thin_route, the
one function the conv entry points and the launcher of csrc/conv_thin.hip read).

- A sweep of the query over layers, maps, forms, activations and dtypes answers exactly thin_cover.KERNELS -- the 144 instantiations
  conv_thin.hip compiles -- and gives every layer outside the implicit GEMM some kernel.
- Every case of thin_cover.CASES answers its own kernel, at the default grid caps and at caps of 2; every reachable instantiation has a case.
- At caps of 2 every EXPAND and REDUCE case runs at least two blocks, makes at least one full four-pass trip and at least one tail pass, and
  its pixel count is no multiple of the pixels of a block pass; at the default caps the same cases make one pass.
- The route of the layers the model runs, and what the query refuses."""
import ctypes
import itertools

import pytest

from tests import cover_bounds as B
from tests import thin_cover as C

CHANNELS = (1, 2, 3, 4, 8, 16, 32, 64, 96, 128, 256, 512)


@pytest.fixture(scope="module")
def lib():
    from gansynth_amd import _lib
    assert (_lib.GS_F32, _lib.GS_BF16) == (C.F32, C.BF16) and _lib.THIN_ROUTE_INTS == len(C.ROUTE_FIELDS)
    assert (_lib.THIN_EXPAND, _lib.THIN_REDUCE, _lib.THIN_EXPAND_PNBWD, _lib.THIN_SINGLE3, _lib.THIN_SINGLE, _lib.THIN_DIRECT) == tuple(range(6))
    return _lib.load()


def _igemm(ks, ick, ock, dtype, map_, form, act):
    """conv_shared.h: igemm_supported; gs_conv_fwd alone leaves the implicit GEMM for a tanh behind the conv."""
    return ks == 3 and ick % (16 if dtype == C.F32 else 32) == 0 and ock % 32 == 0 and not (map_ == C.CONV_FWD and form == C.PLAIN and act == C.TANH)


def _asked(map_, form, act, transposed):
    """The (map, form, activation) combinations an entry point has; the query refuses the others."""
    if form == C.FWD_MASK:
        return map_ == C.CONV_FWD and not transposed
    return form == C.PLAIN or (map_ == C.CONV_BWD_DATA and act != C.TANH)


def test_sweep_answers_exactly_the_compiled_kernels(lib):
    seen = set()
    for ks, stride, transposed in ((1, 1, 0), (3, 1, 0), (3, 2, 0), (3, 2, 1)):
        for ci, co, dtype, map_ in itertools.product(CHANNELS, CHANNELS, (C.F32, C.BF16), (C.CONV_FWD, C.CONV_BWD_DATA)):
            ick, ock = (ci, co) if map_ == C.CONV_FWD else (co, ci)
            for form, act in itertools.product((C.PLAIN, C.FWD_MASK, C.BWD_PNBWD), (C.NONE, C.LRELU, C.TANH)):
                if not _asked(map_, form, act, transposed):
                    continue
                r = C.query(lib, (2, 6, 10, ci, co, ks, stride, transposed), dtype, map_, form, act, act != C.NONE, C.LRELU if form == C.FWD_MASK else C.NONE, False)
                assert (r is None) == _igemm(ks, ick, ock, dtype, map_, form, act), (ks, stride, transposed, ci, co, dtype, map_, form, act, r)
                if r is not None:
                    assert 0 <= r.kernel <= C.DIRECT and r.grid >= 1
                    seen.add(C.route_key(r, dtype))
    assert seen == set(C.KERNELS), (sorted(seen - set(C.KERNELS)), sorted(set(C.KERNELS) - seen))


def test_every_case_answers_its_own_kernel(lib):
    for c in C.CASES:
        for caps in (None, C.CAPPED):
            r = C.route(lib, c, caps)
            assert r is not None and C.route_key(r, c.key.dtype) == c.key, (C.case_id(c), caps, r)
    # every instantiation an entry point reaches has a case (gs_conv_fwd_mask asks for no activation: masked EXPAND with one is out of reach)
    reachable = {k for k in C.KERNELS if not (k.kernel == C.EXPAND and k.MASKED and k.ACT)}
    assert {c.key for c in C.CASES} == reachable
    assert len(reachable) == 144 - 16
    assert set(C.families()) >= {(k, d, C.S1) for k in (C.EXPAND, C.REDUCE, C.EXPAND_PNBWD) for d in (C.F32, C.BF16)}
    assert set(C.families()) >= {(k, d, m) for k in (C.SINGLE3, C.SINGLE, C.DIRECT) for d in (C.F32, C.BF16) for m in (C.S1, C.S2, C.T2)}


def test_capped_cases_make_full_trips_and_tail_passes(lib):
    n = 0
    for c in C.CASES:
        if c.key.kernel not in (C.EXPAND, C.REDUCE):
            continue
        n += 1
        pixels = c.n * c.h * c.w
        r = C.route(lib, c, C.CAPPED)
        assert r.grid == 2 and r.trips >= 1 and r.tails >= 1 and pixels % r.ppb != 0, (C.case_id(c), r)
        r = C.route(lib, c, (2048, 4096))
        assert r.grid >= 2 and (r.trips, r.tails) == (0, 1) and r.grid == -(-pixels // r.ppb), (C.case_id(c), r)
        if c.key.kernel == C.REDUCE and c.key.LC == 4:
            assert C.route(lib, c, C.CAPPED).trips >= 1   # the finishing path of the generator's colour block
    assert n >= 2 * (12 + 36)


def test_the_routes_of_the_model_and_the_passes_left_open(lib):
    top = (8, 128, 1024)
    # generator, top level: 32 -> 2 with tanh and a bias in the kernel; discriminator: 2 -> 32 with leaky relu, bias and the sign words
    r = C.query(lib, top + (32, 2, 1, 1, 0), C.BF16, C.CONV_FWD, C.PLAIN, C.TANH, True, C.NONE, False)
    assert r[:7] == (C.REDUCE, 2, C.TANH, 0, 4, 0, 0) and (r.grid, r.ppb, r.trips, r.tails) == (4096, 64, 1, 0) and (r.epilogue_fused, r.mask_fused, r.bits_fused) == (1, 0, 0)
    r = C.query(lib, top + (2, 32, 1, 1, 0), C.BF16, C.CONV_FWD, C.PLAIN, C.LRELU, True, C.NONE, True)
    assert r[:7] == (C.EXPAND, 2, C.LRELU, 0, 0, 0, 0) and (r.grid, r.ppb, r.trips, r.tails) == (2048, 64, 2, 0) and (r.epilogue_fused, r.mask_fused, r.bits_fused) == (1, 0, 1)
    r = C.query(lib, top + (2, 32, 1, 1, 0), C.F32, C.CONV_FWD, C.PLAIN, C.LRELU, True, C.NONE, True)
    assert r.kernel == C.EXPAND and r.bits_fused == 0                                      # (the words go with bf16 results)
    r = C.query(lib, top + (2, 32, 1, 1, 0), C.BF16, C.CONV_FWD, C.FWD_MASK, C.NONE, False, C.LRELU, False)
    assert (r.kernel, r.MASKED, r.epilogue_fused, r.mask_fused) == (C.EXPAND, 1, 0, 1)
    r = C.query(lib, top + (32, 2, 1, 1, 0), C.BF16, C.CONV_FWD, C.FWD_MASK, C.NONE, False, C.LRELU, False)
    assert (r.kernel, r.MASKED, r.mask_fused) == (C.REDUCE, 0, 0)                          # (the mask: a pass behind the kernel)
    r = C.query(lib, top + (32, 2, 1, 1, 0), C.BF16, C.CONV_BWD_DATA, C.BWD_PNBWD, C.LRELU, False, C.NONE, False)
    assert (r.kernel, r.C, r.grid, r.tails, r.epilogue_fused) == (C.EXPAND_PNBWD, 2, 4096, 4, 1)
    from gansynth_amd import _lib
    for ci, want in ((32, 1), (512, 1), (1024, 0), (48, 0)):   # up to 64 lanes per pixel, a power of two
        conv = _lib.GsConv(2, 8, 16, ci, 2, 1, 1, 0, C.BF16, 0, 1.0, None, 0)
        assert lib.gs_conv_bwd_data_pnbwd_is_fused(conv) == want, ci
        r = C.query(lib, (2, 8, 16, ci, 2, 1, 1, 0), C.BF16, C.CONV_BWD_DATA, C.BWD_PNBWD, C.NONE, False, C.NONE, False)
        assert r.epilogue_fused == want and (r.kernel == C.EXPAND_PNBWD) == bool(want), (ci, r)
    # the stddev plane of the last discriminator block and the whole 257-channel conv
    r = C.query(lib, (8, 2, 16, 1, 256, 3, 1, 0), C.BF16, C.CONV_BWD_DATA, C.PLAIN, C.NONE, False, C.NONE, False)
    assert (r.kernel, r.grid, r.ppb) == (C.SINGLE3, 64, 4)
    r = C.query(lib, (8, 2, 16, 257, 256, 3, 1, 0), C.BF16, C.CONV_FWD, C.PLAIN, C.LRELU, True, C.NONE, True)
    assert (r.kernel, r.OCV, r.VEC, r.grid) == (C.DIRECT, 4, 1, 64) and (r.epilogue_fused, r.bits_fused) == (1, 0)   # (bias and leaky relu on the fp32 sum)
    # a tanh behind a 3x3 layer of the implicit GEMM's channel counts runs here
    assert C.query(lib, (2, 8, 16, 64, 64, 3, 1, 0), C.BF16, C.CONV_FWD, C.PLAIN, C.LRELU, True, C.NONE, False) is None
    assert C.query(lib, (2, 8, 16, 64, 64, 3, 1, 0), C.BF16, C.CONV_FWD, C.PLAIN, C.TANH, True, C.NONE, False).kernel == C.DIRECT


def test_query_refusals(lib):
    from gansynth_amd import _lib
    out = (ctypes.c_int * _lib.THIN_ROUTE_INTS)()
    good = _lib.GsConv(2, 8, 16, 2, 32, 1, 1, 0, C.BF16, 0, 1.0, None, 0)
    assert lib.gs_conv_thin_route(good, C.CONV_FWD, C.PLAIN, C.NONE, 0, 0, 0, None, out) == 0
    assert lib.gs_conv_thin_route(good, 2, C.PLAIN, C.NONE, 0, 0, 0, None, out) == -1 and b"map" in lib.gs_last_error()
    assert lib.gs_conv_thin_route(good, C.CONV_FWD, 3, C.NONE, 0, 0, 0, None, out) == -1
    assert lib.gs_conv_thin_route(good, C.CONV_FWD, C.PLAIN, 3, 0, 0, 0, None, out) == -1 and b"activation" in lib.gs_last_error()
    assert lib.gs_conv_thin_route(good, C.CONV_FWD, C.PLAIN, C.NONE, 0, 0, 0, (ctypes.c_int * 2)(0, 2), out) == -1 and b"caps" in lib.gs_last_error()
    assert lib.gs_conv_thin_route(good, C.CONV_FWD, C.PLAIN, C.NONE, 0, 0, 0, None, None) == -1
    # combinations no entry point has
    assert lib.gs_conv_thin_route(good, C.CONV_BWD_DATA, C.FWD_MASK, C.NONE, 0, C.LRELU, 0, None, out) == -1 and b"masked forward" in lib.gs_last_error()
    assert lib.gs_conv_thin_route(good, C.CONV_FWD, C.BWD_PNBWD, C.NONE, 0, 0, 0, None, out) == -1 and b"data gradient" in lib.gs_last_error()
    assert lib.gs_conv_thin_route(good, C.CONV_BWD_DATA, C.BWD_PNBWD, C.TANH, 0, 0, 0, None, out) == -1
    up = _lib.GsConv(2, 8, 16, 4, 4, 3, 2, 1, C.BF16, 0, 1.0, None, 0)
    assert lib.gs_conv_thin_route(up, C.CONV_FWD, C.FWD_MASK, C.NONE, 0, C.LRELU, 0, None, out) == -1
    # a tanh moves only gs_conv_fwd off the implicit GEMM: the data gradient of a 64 -> 64 3x3 layer stays there whatever `act` says
    big = _lib.GsConv(2, 8, 16, 64, 64, 3, 1, 0, C.BF16, 0, 1.0, None, 0)
    assert lib.gs_conv_thin_route(big, C.CONV_BWD_DATA, C.PLAIN, C.TANH, 0, 0, 0, None, out) == 0 and out[0] == -1
    assert lib.gs_conv_thin_route(big, C.CONV_FWD, C.FWD_MASK, C.TANH, 0, C.LRELU, 0, None, out) == 0 and out[0] == -1
    assert lib.gs_conv_thin_route(big, C.CONV_FWD, C.PLAIN, C.TANH, 0, 0, 0, None, out) == 0 and out[0] == C.DIRECT
    assert lib.gs_conv_thin_route(_lib.GsConv(2, 8, 16, 2, 32, 5, 1, 0, C.BF16, 0, 1.0, None, 0), C.CONV_FWD, C.PLAIN, C.NONE, 0, 0, 0, None, out) == -1


# ------------------------------------------------------------------------------------------------ the element-wise bound (tests/cover_bounds.py)
def test_table_is_the_constants_and_the_bound_is_never_weaker():
    """The docstring's table is CEILINGS (one family per kernel), every ceiling is what the rule gives for its measurement, and the bound at its
    largest stays under the max-norm tolerance these cases were held to before: for every dtype, number of roundings and a forward tanh."""
    B.check_table(C.__doc__, C.CEILINGS)
    assert set(C.CEILINGS) == set(C.KERNEL_NAMES)
    for family, (measured, suite, here) in C.CEILINGS.items():
        assert suite == C.TOLERANCE[C.F32]
        for dtype, r in ((C.F32, 0), (C.BF16, 1), (C.BF16, 2)):
            for tanh_fwd in (False, True):
                assert B.never_weaker(C.TOLERANCE[dtype], here, r, tanh_fwd), (family, dtype, r, tanh_fwd)


def _routed(lib):
    for c in C.CASES:
        assert C.macs(c) <= B.SMALL_MACS, C.case_id(c)   # every case runs at all twelve seeds of the measurement
        yield c, C.route(lib, c)


def test_roundings_follow_the_route(lib):
    """A bf16 result is rounded twice exactly where the route leaves a pass behind the kernel, and the only pass any case leaves is a mask
    (the REDUCE kernel's masked forward, the masked data gradients of the EXPAND and direct kernels): bias and activation ride in every kernel, on the fp32 sum.
    (As a pass of their own behind the direct and single kernels they added the bias to a sum already rounded to bf16, and where the two
    cancel that rounding was up to 240 times this bound: the measurement of tests/thin_cover.py's docstring.)"""
    twice = {c for c, r in _routed(lib) if C.roundings(c, r) == 2}
    assert twice and all(c.key.dtype == C.BF16 and c.mask_act and not (c.bias or c.act) for c in twice)
    assert {c.key.kernel for c in twice} == {C.DIRECT, C.REDUCE, C.EXPAND}
    for c, r in _routed(lib):
        assert r.epilogue_fused == int(bool(c.bias or c.act) or c.call == "pnbwd"), C.case_id(c)
        assert C.roundings(c, r) == C.roundings(c, C.route(lib, c, C.CAPPED)), C.case_id(c)
        assert C.roundings(c, r) == (0 if c.key.dtype == C.F32 else 1 + int(bool(c.mask_act) and not r.mask_fused)), C.case_id(c)


def test_an_honest_kernel_is_inside_the_bound(lib):
    """The map restated in fp32 on the operands as stored (torch on the CPU; bias, activation and mask in fp32, one store in the case's dtype)
    stays inside the bound at every case."""
    worst = {}
    for c, r in _routed(lib):
        d = C.inputs(c)
        ref, mag = C.reference(c, d), C.mag(c, d)
        m = B.measure(C.case_id(c), C.restated(c, d), ref, C.bound(c, r, ref, mag), mag)
        assert m.over == 0 and m.compared == ref.numel() and m.worst <= 1, m.message
        worst[c.key.dtype] = max(worst.get(c.key.dtype, 0.0), m.worst)
    print(f"{len(C.CASES)} honest results, worst err / bound per dtype (fp32, bf16): {worst}")
    assert set(worst) == {C.F32, C.BF16}


def test_subtly_wrong_kernels_pass_the_old_assertion_and_fail_the_bound(lib):
    """M1 (bf16 cases that contract more than one channel): two K partials each rounded to bf16 before the last add, in front of bias,
    activation and mask; M3 (bf16 cases rounded once: a bound that admits two roundings admits one truncation): a truncating store; M5 (every
    case): every element under 5 % of the largest scaled by 1 + 2^-6."""
    gap = B.Gap(("M1", "M3", "M5"))
    for c, r in _routed(lib):
        d = C.inputs(c)
        ref, mag = C.reference(c, d), C.mag(c, d)
        bnd, tag, old = C.bound(c, r, ref, mag), C.case_id(c), C.TOLERANCE[c.key.dtype]
        if c.key.dtype == C.F32:
            gap.check("M5", tag, B.stored_as(B.scale_small(ref), bf16=False), ref, bnd, old)
            continue
        gap.check("M5", tag, B.stored_as(B.scale_small(ref), bf16=True), ref, bnd, old)
        if C.roundings(c, r) == 1:
            gap.check("M3", tag, B.bf16_truncate(ref), ref, bnd, old)
        axis = 3 if c.call in ("bwd_data", "bwd_data_t", "pnbwd") else 2   # the contracted side of the HWIO weight
        half = d["w"].shape[axis] // 2
        if half:
            lo, hi = d["w"].clone(), d["w"].clone()
            lo.narrow(axis, half, d["w"].shape[axis] - half).zero_()
            hi.narrow(axis, 0, half).zero_()
            y = B.fold_through_bf16(d["alpha"] * C.conv64(c, d["a"], lo), d["alpha"] * C.conv64(c, d["a"], hi))
            gap.check("M1", tag, B.bf16_rne(C.finish(c, d, y)), ref, bnd, old)
    gap.close()
