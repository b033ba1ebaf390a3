"""CPU: the cases of tests/test_dense_cover_gpu.py exist and mean something (no GPU: gs_dense_route is host arithmetic on dense_route, the one
function the three dense entry points and gs_dense_fwd_workspace_bytes read).

- On a grid of batch sizes x input widths x output widths on both sides of every threshold of the conditions, with and without a channels-last
  factorisation, for both dtypes, both knob values and the three maps, the library's route equals dense_cover.route_py, refusals included, and its
  ws_bytes is what gs_dense_fwd_workspace_bytes answers.
- Every case of dense_cover.CASES answers its own instantiation under its own knob; the 36 instantiations all have a case; the finalize pass
  sees a tail alone, a trip and a tail, and whole trips.
- The routes of the layers the model runs are those of the commit before the route existed (read off its conditions by hand)."""
import itertools

import pytest

from tests import cover_bounds as B
from tests import dense_cover as C

BATCHES = (1, 5, 8, 13, 16, 17, 24, 30, 64, 65)
# every threshold of the conditions with the divisors that meet it there
_THRESHOLDS = {4: (4,), 16: (4, 16), 32: (4, 32), 64: (32, 64), 128: (4, 128), 256: (32, 64, 256), 1024: (4, 16, 64), 2048: (4, 64, 256), 4096: (16, 256)}
WIDTHS = sorted({v for t, ds in _THRESHOLDS.items() for v in [t - 1, t, t + 1] + [t - d for d in ds] + [t + d for d in ds] if v > 0})


def factorisation(inp):
    """A channels-last (c, hw) of an input width, or None where it has no divisor to offer: 4 or 8 channels, else the smallest factor."""
    c = next((f for f in (8, 4, 2, 3, 5, 7, 11, 13) if inp % f == 0 and inp // f > 1), None)
    return None if c is None else (c, inp // c)


@pytest.fixture(scope="module")
def lib():
    from gansynth_amd import _lib
    assert (_lib.GS_F32, _lib.GS_BF16) == (C.F32, C.BF16) and _lib.DENSE_ROUTE_INTS == len(C.ROUTE_FIELDS) + 1
    assert (_lib.DENSE_FWD, _lib.DENSE_FWD_SMALL, _lib.DENSE_FWD_FAST, _lib.DENSE_FWD_MFMA, _lib.DENSE_FINALIZE, _lib.DENSE_BWD_DATA, _lib.DENSE_BWD_DATA_WIDE,
            _lib.DENSE_BWD_DATA_FAST, _lib.DENSE_BWD_DATA_MFMA, _lib.DENSE_BWD_WEIGHT, _lib.DENSE_BWD_WEIGHT_FAST) == tuple(range(11))
    assert (_lib.DENSE_MAP_FWD, _lib.DENSE_MAP_BWD_DATA, _lib.DENSE_MAP_BWD_WEIGHT) == (C.FWD_MAP, C.BWD_DATA_MAP, C.BWD_WEIGHT_MAP)
    return _lib.load()


def test_route_equals_the_restatement_on_the_threshold_grid(lib):
    import ctypes
    import os
    assert "GS_NO_DENSE_MFMA" not in os.environ, "gs_dense_fwd_workspace_bytes reads the process's knob: unset here"
    from gansynth_amd import _lib
    ints = (ctypes.c_int * _lib.DENSE_ROUTE_INTS)()
    d = _lib.GsDense(1, 1, 1, 0, 0, 0, 1.0, None, 0)
    n, seen, refused = 0, set(), 0
    for inp in WIDTHS:
        for rc, rhw in {(0, 0), factorisation(inp) or (0, 0)}:
            for b, out, no_mfma, map_ in itertools.product(BATCHES, WIDTHS, (0, 1), (C.FWD_MAP, C.BWD_DATA_MAP, C.BWD_WEIGHT_MAP)):
                want = C.route_py(map_, b, inp, out, rc, rhw, no_mfma)
                d.b, d.inp, d.out, d.c, d.hw = b, inp, out, rc, rhw
                for dtype in (C.F32, C.BF16):
                    d.dtype = dtype
                    code = lib.gs_dense_route(d, map_, no_mfma, ints)
                    got = code if code else C.Route(*ints[:10], (ints[10] & 0xFFFFFFFF) | (ints[11] << 32))
                    assert got == want, (map_, b, inp, out, rc, rhw, dtype, no_mfma, got, want)
                    n += 1
                if isinstance(want, int):
                    refused += 1
                    continue
                seen.add((want.kernel, want.FB, want.WPR))
                if map_ == C.FWD_MAP and no_mfma == 0:
                    assert lib.gs_dense_fwd_workspace_bytes(d) == want.ws_bytes, (b, inp, out, rc, rhw)
    assert seen == {(k.kernel, k.FB, k.WPR) for k in C.KERNELS if k.kernel != C.FINALIZE} and refused > 0 and n > 100000


def test_every_case_answers_its_own_kernel(lib):
    import os
    assert "GS_NO_DENSE_MFMA" not in os.environ
    for c in C.CASES:
        r = C.route(lib, c)
        assert not isinstance(r, int) and C.route_key(r, c.key.dtype) == c.key, (C.case_id(c), r)
        assert r == C.route_py(c.map, c.b, c.inp, c.out, c.c, c.hw, c.no_mfma)
        assert (r.finalize, r.ksplit if r.finalize else 0) == (int(c.fin > 0), c.fin), (C.case_id(c), r)
        if not c.no_mfma:   # what this process's environment gives
            assert C.route(lib, c, no_mfma=-1) == r
        if c.key.kernel in (C.FWD_MFMA, C.BWD_DATA_MFMA):   # every MFMA case has a twin under the knob
            twin = c._replace(no_mfma=1)
            assert any(o._replace(key=c.key, fin=c.fin) == twin for o in C.CASES), C.case_id(c)
    covered = set().union(*(C.case_keys(c) for c in C.CASES))
    assert covered == set(C.KERNELS), (sorted(set(C.KERNELS) - covered), sorted(covered - set(C.KERNELS)))
    assert set(C.families()) == {(k.kernel, k.dtype) for k in C.KERNELS}
    for d in (C.F32, C.BF16):   # the finalize pass: a tail alone, a trip and a tail, whole trips
        fins = {c.fin for c in C.CASES if c.fin and c.key.dtype == d}
        assert all(fins & set(v) for v in C.FIN_KINDS.values()) and fins <= set().union(*C.FIN_KINDS.values()), fins
    # what the cases are there for: ragged single passes, second passes, the row map in every kernel that has one
    by = {}
    for c in C.CASES:
        by.setdefault(c.key.kernel, []).append(c)
    assert all(any(c.c for c in by[k]) for k in (C.FWD_FAST, C.FWD_MFMA, C.BWD_DATA_FAST, C.BWD_DATA_MFMA, C.BWD_WEIGHT_FAST))
    assert all(any(C.route(lib, c).passes == 2 for c in by[k]) for k in (C.FWD, C.FWD_FAST, C.BWD_DATA, C.BWD_DATA_FAST, C.BWD_DATA_WIDE))
    assert any(c.c == 8 and not c.no_mfma for c in by[C.FWD_MFMA])   # 8 rows per column block: the map wraps inside a lane's 16-row run
    assert all({c.accumulate for c in by[k]} == {False, True} for k in (C.BWD_WEIGHT, C.BWD_WEIGHT_FAST))


# (map, b, in, out, c, hw) -> (kernel, FB, WPR, step, passes, grid_x, grid_y, ksplit, ipb, finalize, ws_bytes) of the model's layers, knob unset
_MODEL = [
    # generator 512 -> 8192
    ((C.FWD_MAP, 8, 512, 8192, 0, 0), (C.FWD_FAST, 8, 0, 8, 1, 256, 1, 1, 512, 0, 8 * 8192 * 4)),
    ((C.FWD_MAP, 16, 512, 8192, 0, 0), (C.FWD_FAST, 16, 0, 16, 1, 256, 1, 1, 512, 0, 16 * 8192 * 4)),
    ((C.BWD_DATA_MAP, 8, 512, 8192, 0, 0), (C.BWD_DATA_FAST, 8, 4, 8, 1, 512, 1, 0, 0, 0, 0)),
    ((C.BWD_DATA_MAP, 16, 512, 8192, 0, 0), (C.BWD_DATA_FAST, 16, 4, 16, 1, 512, 1, 0, 0, 0, 0)),
    ((C.BWD_WEIGHT_MAP, 8, 512, 8192, 0, 0), (C.BWD_WEIGHT_FAST, 0, 0, 8, 1, 32, 32, 0, 0, 0, 0)),
    ((C.BWD_WEIGHT_MAP, 16, 512, 8192, 0, 0), (C.BWD_WEIGHT_FAST, 0, 0, 16, 1, 32, 32, 0, 0, 0, 0)),
    # discriminator 8192 -> 256 on the channels-last 256 x (2 x 16) activation
    ((C.FWD_MAP, 8, 8192, 256, 256, 32), (C.FWD_MFMA, 0, 0, 8, 1, 128, 1, 128, 64, 1, 128 * 8 * 256 * 4)),
    ((C.FWD_MAP, 16, 8192, 256, 256, 32), (C.FWD_MFMA, 0, 0, 16, 1, 128, 1, 128, 64, 1, 128 * 16 * 256 * 4)),
    ((C.FWD_MAP, 24, 8192, 256, 256, 32), (C.FWD_MFMA, 0, 0, 24, 1, 128, 1, 128, 64, 1, 128 * 24 * 256 * 4)),
    ((C.BWD_DATA_MAP, 8, 8192, 256, 256, 32), (C.BWD_DATA_MFMA, 0, 0, 8, 1, 128, 1, 0, 0, 0, 0)),
    ((C.BWD_DATA_MAP, 16, 8192, 256, 256, 32), (C.BWD_DATA_MFMA, 0, 0, 16, 1, 128, 1, 0, 0, 0, 0)),
    ((C.BWD_DATA_MAP, 24, 8192, 256, 256, 32), (C.BWD_DATA_MFMA, 0, 0, 24, 1, 128, 1, 0, 0, 0, 0)),
    ((C.BWD_WEIGHT_MAP, 8, 8192, 256, 256, 32), (C.BWD_WEIGHT_FAST, 0, 0, 8, 1, 1, 512, 0, 0, 0, 0)),
    ((C.BWD_WEIGHT_MAP, 16, 8192, 256, 256, 32), (C.BWD_WEIGHT_FAST, 0, 0, 16, 1, 1, 512, 0, 0, 0, 0)),
    ((C.BWD_WEIGHT_MAP, 24, 8192, 256, 256, 32), C.ERR_UNSUPPORTED),   # (24 rows reach the layer flattened: kernels.dense_nhwc_ok)
    ((C.BWD_WEIGHT_MAP, 24, 8192, 256, 0, 0), (C.BWD_WEIGHT, 0, 0, 24, 1, 8192, 1, 0, 0, 0, 0)),
    # logits 256 -> 61; the classifier's 64-row call
    ((C.FWD_MAP, 8, 256, 61, 0, 0), (C.FWD_SMALL, 0, 0, 8, 1, 1, 8, 1, 256, 0, 8 * 8 * 61 * 4)),
    ((C.FWD_MAP, 16, 256, 61, 0, 0), (C.FWD_SMALL, 0, 0, 16, 1, 1, 16, 1, 256, 0, 8 * 16 * 61 * 4)),
    ((C.FWD_MAP, 64, 256, 61, 0, 0), (C.FWD_SMALL, 0, 0, 64, 1, 1, 64, 1, 256, 0, 8 * 64 * 61 * 4)),
    ((C.BWD_DATA_MAP, 8, 256, 61, 0, 0), (C.BWD_DATA, 0, 0, 16, 1, 64, 1, 0, 0, 0, 0)),
    ((C.BWD_DATA_MAP, 16, 256, 61, 0, 0), (C.BWD_DATA, 0, 0, 16, 1, 64, 1, 0, 0, 0, 0)),
    ((C.BWD_DATA_MAP, 64, 256, 61, 0, 0), (C.BWD_DATA, 0, 0, 16, 4, 64, 1, 0, 0, 0, 0)),
    ((C.BWD_WEIGHT_MAP, 8, 256, 61, 0, 0), (C.BWD_WEIGHT, 0, 0, 8, 1, 61, 1, 0, 0, 0, 0)),
    ((C.BWD_WEIGHT_MAP, 16, 256, 61, 0, 0), (C.BWD_WEIGHT, 0, 0, 16, 1, 61, 1, 0, 0, 0, 0)),
    ((C.BWD_WEIGHT_MAP, 64, 256, 61, 0, 0), (C.BWD_WEIGHT, 0, 0, 64, 1, 61, 1, 0, 0, 0, 0)),
]


def test_the_routes_of_the_model(lib):
    for (map_, b, inp, out, c, hw), want in _MODEL:
        for dtype in (C.F32, C.BF16):
            got = C.query(lib, map_, b, inp, out, c, hw, dtype)
            assert got == (want if isinstance(want, int) else C.Route(*want)), (map_, b, inp, out, c, hw, dtype, got)


def test_query_refusals(lib):
    import ctypes
    from gansynth_amd import _lib
    ints = (ctypes.c_int * _lib.DENSE_ROUTE_INTS)()
    good = _lib.GsDense(8, 8192, 256, 256, 32, C.BF16, 1.0, None, 0)
    assert lib.gs_dense_route(good, C.FWD_MAP, -1, ints) == 0
    assert lib.gs_dense_route(good, 3, -1, ints) == -1 and b"map" in lib.gs_last_error()
    assert lib.gs_dense_route(good, C.FWD_MAP, -1, None) == -1
    assert lib.gs_dense_route(None, C.FWD_MAP, -1, ints) == -1 and b"descriptor" in lib.gs_last_error()
    assert lib.gs_dense_route(_lib.GsDense(8, 8192, 256, 256, 32, 2, 1.0, None, 0), C.FWD_MAP, -1, ints) == -1 and b"dtype" in lib.gs_last_error()
    assert lib.gs_dense_route(_lib.GsDense(8, 8192, 256, 256, 31, C.BF16, 1.0, None, 0), C.FWD_MAP, -1, ints) == -1 and b"wide" in lib.gs_last_error()
    assert lib.gs_dense_route(_lib.GsDense(0, 8192, 256, 0, 0, C.BF16, 1.0, None, 0), C.FWD_MAP, -1, ints) == -1
    # what the entry points refuse, with their code -- before anything is dereferenced or launched
    P = 0x10000
    odd = _lib.GsDense(8, 8190, 256, 2, 4095, C.BF16, 1.0, None, 0)
    assert lib.gs_dense_route(odd, C.FWD_MAP, -1, ints) == -3 and lib.gs_dense_fwd(odd, P, P, None, 0, P, None) == -3 and b"in % 4" in lib.gs_last_error()
    assert lib.gs_dense_fwd_workspace_bytes(odd) == 0
    narrow = _lib.GsDense(8, 8192, 61, 256, 32, C.BF16, 1.0, None, 0)
    assert lib.gs_dense_route(narrow, C.BWD_DATA_MAP, -1, ints) == -3 and lib.gs_dense_bwd_data(narrow, P, P, P, None) == -3 and b"out % 256" in lib.gs_last_error()
    tall = _lib.GsDense(17, 8192, 256, 256, 32, C.BF16, 1.0, None, 0)
    assert lib.gs_dense_route(tall, C.BWD_WEIGHT_MAP, -1, ints) == -3 and lib.gs_dense_bwd_weight(tall, P, P, P, 0, None) == -3 and b"batch <= 16" in lib.gs_last_error()
    assert lib.gs_dense_fwd(good, P, P, None, 3, P, None) == -1 and b"activation" in lib.gs_last_error()
    assert lib.gs_dense_fwd(good, P, P, None, 0, P, None) == -4 and b"workspace" in lib.gs_last_error()   # (ws_bytes 0 against 128 slices of partials)


# ------------------------------------------------------------------------------------------------ the element-wise bound (tests/cover_bounds.py)
def test_table_is_the_constants_and_the_bound_is_never_weaker():
    """The docstring's table is CEILINGS (one family per kernel but the finalize pass, which rides), every ceiling is what the rule gives for its
    measurement, and the bound at its largest stays under the max-norm tolerance each (map, dtype) was held to before."""
    B.check_table(C.__doc__, C.CEILINGS)
    assert set(C.CEILINGS) == set(C.KERNEL_NAMES) - {"finalize"}
    for c in C.CASES:
        measured, suite, here = C.CEILINGS[C.family(c)]
        assert suite == C.TOLERANCE[c.map][C.F32]
        assert B.never_weaker(C.TOLERANCE[c.map][c.key.dtype], here, C.roundings(c), c.act == C.TANH), C.case_id(c)
        assert C.macs(c) <= B.SMALL_MACS, C.case_id(c)   # every case runs at all twelve seeds of the measurement
        assert C.products(c) == {C.FWD_MAP: c.inp, C.BWD_DATA_MAP: c.out, C.BWD_WEIGHT_MAP: c.b}[c.map]


def test_an_honest_kernel_is_inside_the_bound():
    """The map restated in fp32 on the operands as stored (torch's CPU matmul; bias, activation and accumulate in fp32, one store in the result's
    dtype) stays inside the bound at every case."""
    worst = {}
    for c in C.CASES:
        d = C.inputs(c)
        ref, mag = C.reference(c, d), C.mag(c, d)
        m = B.measure(C.case_id(c), C.restated(c, d), ref, C.bound(c, ref, mag), mag)
        assert m.over == 0 and m.compared == ref.numel() and m.worst <= 1, m.message
        worst[(c.map, c.key.dtype)] = max(worst.get((c.map, c.key.dtype), 0.0), m.worst)
    print(f"{len(C.CASES)} honest results, worst err / bound per (map, dtype): {worst}")
    assert len(worst) == 6


def test_subtly_wrong_kernels_pass_the_old_assertion_and_fail_the_bound():
    """M1 (bf16 results): two K partials each rounded to bf16 before the last add, in front of bias and activation; M3 (bf16 results): a
    truncating store; M5 (every case, the fp32 weight gradients among them): every element under 5 % of the largest scaled by 1 + 2^-6."""
    import torch
    gap = B.Gap(("M1", "M3", "M5"))
    for c in C.CASES:
        d = C.inputs(c)
        ref, mag = C.reference(c, d), C.mag(c, d)
        bnd, tag, old = C.bound(c, ref, mag), C.case_id(c), C.TOLERANCE[c.map][c.key.dtype]
        if not C.roundings(c):
            gap.check("M5", tag, B.stored_as(B.scale_small(ref), bf16=False), ref, bnd, old)
            continue
        gap.check("M5", tag, B.stored_as(B.scale_small(ref), bf16=True), ref, bnd, old)
        gap.check("M3", tag, B.bf16_truncate(ref), ref, bnd, old)
        axis = 0 if c.map == C.FWD_MAP else 1   # the contracted side of the [in, out] weight
        half = d["w"].shape[axis] // 2
        lo, hi = d["w"].clone(), d["w"].clone()
        lo.narrow(axis, half, d["w"].shape[axis] - half).zero_()
        hi.narrow(axis, 0, half).zero_()
        parts = [C.reference(c._replace(bias=False, act=C.NONE), dict(d, w=w)) for w in (lo, hi)]
        y = B.fold_through_bf16(*parts)
        if c.bias:
            y = y + d["bias"].double()
        y = torch.tanh(y) if c.act == C.TANH else (torch.where(y > 0, y, 0.2 * y) if c.act == C.LRELU else y)
        gap.check("M1", tag, B.bf16_rne(y), ref, bnd, old)
    gap.close()
