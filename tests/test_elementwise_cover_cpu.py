"""CPU: the cases of tests/test_elementwise_cover_gpu.py exist and mean something (no GPU: gs_elementwise_route is host arithmetic on
elementwise_route, the one function the entry points of csrc/elementwise.hip, the batch-stddev entry points of csrc/small_ops.hip,
gs_channel_sum_workspace_bytes, gs_pixel_norm_bwd_bias_workspace_bytes and gs_bias_partial_rows read).

- On a grid of rows x channels x block factors on both sides of every threshold of the conditions (4, 8, 64, 256, 1024, c % 4, powers of two,
  p * c % 8, fy * fx = 32, 64 and 2048 partial rows, both grid caps), for both dtypes and three settings of the caps, the library's route equals
  elementwise_cover.route_py, refusals included; the workspace functions and gs_bias_partial_rows give the route's figures.
- Every case of elementwise_cover.CASES answers its own instantiation and the path it is there for; the 86 instantiations are exactly what the
  sweep reaches and all have a case; pixel norm runs every L in 1..64 in both dtypes, plain and with the bias sums; under the GPU test's knobs
  every grid-stride kernel has a case whose loop takes a second trip.
- The routes of the shapes the model runs are those of the commit before the route existed (read off its conditions by hand).
- The measure sees the errors it is there for: a float64 result that is wrong in one row, one channel shift or one element lands above the
  ceiling of its family; the right one rounded to the case's dtype lands below."""
import ctypes
import itertools
import os

import pytest
import torch

from tests import elementwise_cover as C

ROWS = sorted({v for t in (1, 4, 8, 64, 256, 1024, 2048, 64 * 8 * 64, 2048 * 8, 8192 * 256, 8192 * 256 * 4, 1024 * 512) for v in (t - 1, t, t + 1) if v > 0}
              | {5, 37, 70, 77, 300, 700, 16700, 2 ** 23 + 5})
CHANNELS = (1, 2, 3, 4, 5, 7, 8, 9, 12, 15, 16, 17, 31, 32, 33, 48, 61, 63, 64, 65, 127, 128, 129, 255, 256, 257, 260, 261, 300, 511, 512, 513, 1000, 1023,
            1024, 1025, 1028, 2048)
FACTORS = ((1, 1), (2, 2), (3, 2), (31, 1), (1, 31), (4, 8), (8, 4), (3, 11), (5, 7), (8, 8), (9, 9), (64, 64), (0, 2))
CAPS = ((C.EW_CAP, C.PN_BIAS_CAP), (2, 2), (5, 3))
ROWS_COLS_OPS = (C.OP_BIAS_ACT, C.OP_CHANNEL_SUM, C.OP_ACT_BWD_BIAS, C.OP_PN_FWD, C.OP_PN_BWD, C.OP_PN_BWD_BIAS, C.OP_PN_BWD_BWD)
NUMEL_OPS = (C.OP_ACT_BWD, C.OP_TANH_BWD_BWD, C.OP_AXPBY, C.OP_AXPBY_DEV)
STDDEV_OPS = (C.OP_STDDEV_FWD, C.OP_STDDEV_BWD, C.OP_STDDEV_BWD_BWD)
ALL_ARGS = [dict(act=a, bias=b) for a in (0, 1, 2) for b in (0, 1)]   # what a call may ask beyond its shape, where an instantiation hangs on it


@pytest.fixture(scope="module")
def lib():
    from gansynth_amd import _lib
    assert (_lib.GS_F32, _lib.GS_BF16) == (C.F32, C.BF16) and _lib.EW_ROUTE_INTS == len(C.ROUTE_FIELDS) + 1
    assert (_lib.EW_OP_BIAS_ACT, _lib.EW_OP_ACT_BWD, _lib.EW_OP_TANH_BWD_BWD, _lib.EW_OP_AXPBY, _lib.EW_OP_AXPBY_DEV, _lib.EW_OP_UPSCALE, _lib.EW_OP_ROW_SCALE,
            _lib.EW_OP_CHANNEL_SUM, _lib.EW_OP_ACT_BWD_BIAS, _lib.EW_OP_PIXEL_NORM_FWD, _lib.EW_OP_PIXEL_NORM_BWD, _lib.EW_OP_PIXEL_NORM_BWD_BIAS,
            _lib.EW_OP_PIXEL_NORM_BWD_BWD, _lib.EW_OP_BLOCKSUM, _lib.EW_OP_SUMSQ_ROWS, _lib.EW_OP_BATCH_STDDEV_FWD, _lib.EW_OP_BATCH_STDDEV_BWD,
            _lib.EW_OP_BATCH_STDDEV_BWD_BWD) == tuple(range(18)) and len(C.OP_NAMES) == 18
    assert (_lib.EW_BIAS_ACT, _lib.EW_BIAS_ACT_SCALAR, _lib.EW_ACT_BWD, _lib.EW_TANH_BWD_BWD, _lib.EW_AXPBY, _lib.EW_AXPBY_DEV, _lib.EW_UPSCALE, _lib.EW_ROW_SCALE,
            _lib.EW_CHANNEL_SUM, _lib.EW_CHANNEL_SUM_ROWS, _lib.EW_ACT_BWD_SUM, _lib.EW_PIXEL_NORM, _lib.EW_BLOCKSUM, _lib.EW_BLOCKSUM_SMALL, _lib.EW_SUMSQ_ROWS,
            _lib.EW_BATCH_STDDEV_FWD, _lib.EW_BATCH_STDDEV_BWD, _lib.EW_BATCH_STDDEV_BWD_BWD) == tuple(range(18)) and len(C.KERNEL_NAMES) == 18
    assert (_lib.EW_PATH_NONE, _lib.EW_PATH_COLOUR, _lib.EW_PATH_QUADS, _lib.EW_PATH_GENERIC, _lib.EW_PATH_VECTOR, _lib.EW_PATH_SCALAR) == tuple(range(6))
    assert (_lib.ACT_NONE, _lib.ACT_LRELU, _lib.ACT_TANH) == (C.NONE, C.LRELU, C.TANH)
    assert not set(C.KNOBS) & set(os.environ), "the workspace functions and gs_bias_partial_rows read the process's knobs: unset here"
    return _lib.load()


def sweep():
    """(op, p, c, fy, fx) on both sides of every threshold."""
    for op, p, c in itertools.product(ROWS_COLS_OPS, ROWS, CHANNELS):
        yield op, p, c, 0, 0
    for op, p in itertools.product(NUMEL_OPS, ROWS + [0]):
        yield op, p, 0, 0, 0
    for op, p, (fy, fx) in itertools.product((C.OP_UPSCALE, C.OP_BLOCKSUM), ROWS, FACTORS):
        yield op, p, 2, fy, fx
    for op, cols, rows in itertools.product((C.OP_ROW_SCALE, C.OP_SUMSQ_ROWS), ROWS + [0], (0, 1, 2, 3, 8)):
        yield op, cols, 0, rows, 0
    for op, hw, c, b in itertools.product(STDDEV_OPS, (1, 3, 5, 32, 300, 1024), (1, 3, 4, 5, 8, 16, 256), (0, 3, 4, 6, 8, 16)):
        yield op, hw, c, b, 0


def test_route_equals_the_restatement_on_the_threshold_grid(lib):
    from gansynth_amd import _lib
    ints = (ctypes.c_int * _lib.EW_ROUTE_INTS)()
    n, seen, refused, capped = 0, set(), 0, set()
    for (op, p, c, fy, fx), dtype, (ew_cap, pn_cap) in itertools.product(sweep(), C.DTYPES, CAPS):
        want = C.route_py(op, dtype, p, c, fy, fx, ew_cap, pn_cap)
        code = lib.gs_elementwise_route(op, dtype, p, c, fy, fx, ew_cap, pn_cap, ints)
        got = code if code else C.Route(*ints[:16], (ints[16] & 0xFFFFFFFF) | (ints[17] << 32))
        assert got == want, (C.OP_NAMES[op], dtype, p, c, fy, fx, ew_cap, pn_cap, got, want)
        n += 1
        if isinstance(want, int):
            refused += 1
            continue
        for args in ALL_ARGS if want.kernel == C.BIAS_ACT else ([dict(act=1), dict(act=2)] if want.kernel in (C.ACT_BWD, C.ACT_BWD_SUM) or want.two_pass else [{}]):   # (act_bwd has no ACT 0)
            seen |= C.route_keys(op, dtype, want, args)
        if want.kernel in C.GRID_STRIDE and want.grid_x == (pn_cap if op == C.OP_PN_BWD_BIAS else ew_cap) and want.trips > 1:
            capped.add((want.kernel, ew_cap))
        if (ew_cap, pn_cap) != CAPS[0]:
            continue
        # the defaults are this process's environment: the same answer with -1, and the figures of the functions that read the route
        assert lib.gs_elementwise_route(op, dtype, p, c, fy, fx, -1, -1, ints) == 0 and list(ints[:16]) == list(want[:16])
        if op == C.OP_CHANNEL_SUM:
            assert lib.gs_channel_sum_workspace_bytes(p, c) == want.ws_bytes and lib.gs_bias_partial_rows(_lib.BIAS_FROM_CHANNEL_SUM, p, c, dtype) == want.nparts
            assert (want.nparts == 0) == (want.kernel == C.CHANNEL_SUM_ROWS) and (want.levels == 2) == (want.nparts > C.CS_SLAB)
        elif op == C.OP_ACT_BWD_BIAS:
            assert lib.gs_channel_sum_workspace_bytes(p, c) == want.ws_bytes and lib.gs_bias_partial_rows(_lib.BIAS_FROM_ACT_BWD, p, c, dtype) == want.nparts
        elif op == C.OP_PN_BWD_BIAS:
            assert lib.gs_pixel_norm_bwd_bias_workspace_bytes(p, c, dtype) == want.ws_bytes
            assert lib.gs_bias_partial_rows(_lib.BIAS_FROM_PIXEL_NORM_BWD, p, c, dtype) == want.nparts == want.grid_x
        elif op == C.OP_SUMSQ_ROWS:
            assert lib.gs_sumsq_rows_workspace_bytes(fy) == want.ws_bytes
    assert seen == set(C.KERNELS), (sorted(set(C.KERNELS) - seen), sorted(seen - set(C.KERNELS)))
    assert capped == {(k, cap) for k in C.GRID_STRIDE for cap, _ in CAPS}, "both sides of every grid cap"
    assert refused > 0 and n > 50000
    for dtype in C.DTYPES:   # shapes a producer refuses leave no rows and need no workspace
        assert lib.gs_bias_partial_rows(_lib.BIAS_FROM_PIXEL_NORM_BWD, 256, 48, dtype) == 0 and lib.gs_pixel_norm_bwd_bias_workspace_bytes(256, 48, dtype) == 0
        assert lib.gs_bias_partial_rows(3, 256, 32, dtype) == 0 and lib.gs_bias_partial_rows(_lib.BIAS_FROM_CHANNEL_SUM, 0, 32, dtype) == 0


def test_every_case_answers_its_own_kernel(lib):
    covered, by = set(), {}
    for c in C.CASES:
        r = C.route(lib, c)
        assert not isinstance(r, int), C.case_id(c)
        assert r == C.route_py(c.op, c.dtype, *C.words(c.op, c.shape, c.args)), C.case_id(c)
        keys = C.route_keys(c.op, c.dtype, r, c.args)
        assert c.key in keys, (C.case_id(c), C.key_id(c.key), r)
        f = C.facts(c, r)
        assert all(f[k] == v for k, v in c.want.items()), (C.case_id(c), c.want, f)
        covered |= keys
        by.setdefault((r.kernel, c.dtype), []).append((c, r))
        assert sum(t.numel() for t in C.inputs(c).values()) <= 2.2e6, C.case_id(c)   # no case larger than about 2M elements
    assert covered == set(C.KERNELS), (sorted(set(C.KERNELS) - covered), sorted(covered - set(C.KERNELS)))
    assert set(C.families()) == {(k.kernel, k.dtype) for k in C.KERNELS}
    assert len({C.case_id(c) for c in C.CASES}) == len(C.CASES)
    for d in C.DTYPES:
        # pixel norm: every L, plain and with the bias sums; at least two blocks, a ragged last wave where a wave holds several rows, and a
        # partial last trip; with the knobs set two blocks take at least two trips
        for op in (C.OP_PN_FWD, C.OP_PN_BWD, C.OP_PN_BWD_BIAS, C.OP_PN_BWD_BWD):
            mine = [(c, r) for c, r in by[(C.PIXEL_NORM, d)] if c.op == op]
            assert {r.L for _, r in mine} == {1, 2, 4, 8, 16, 32, 64} and {c.shape[1] for c, _ in mine} == set(C.PN_WIDTHS)
            for c, r in mine:
                assert r.grid_x >= 2 and (r.rows == 1 or c.shape[0] % r.rows) and c.shape[0] % (r.grid_x * 4 * r.rows * r.U)
                k = C.route(lib, c, 2, 2)
                assert k.grid_x == 2 and k.trips >= 2 and k[1:7] == r[1:7], C.case_id(c)
        # every grid-stride kernel: a second trip under the knobs of the GPU test's child
        for kernel in C.GRID_STRIDE:
            assert any(C.route(lib, c, 2, 2).trips >= 2 for c, _ in by[(kernel, d)]), (C.KERNEL_NAMES[kernel], d)
        # the tail alone, vectors alone, both
        for kernel in (C.ACT_BWD, C.AXPBY, C.AXPBY_DEV):
            assert {(c.shape[0] >= 4, r.tail) for c, r in by[(kernel, d)]} == {(False, 1), (True, 0), (True, 1)}
        sums = by[(C.CHANNEL_SUM, d)]
        assert {r.path for _, r in sums} == {C.COLOUR, C.QUADS, C.GENERIC} and {r.levels for _, r in sums} == {1, 2}
        assert {c.shape[1] for c, r in sums if r.path == C.COLOUR} == {1, 2, 4} and {2, 4} <= {c.shape[1] for c, r in sums if r.path != C.COLOUR}
        for kernel in (C.CHANNEL_SUM, C.CHANNEL_SUM_ROWS):   # each path with accumulate off and on
            assert all({o.args["accumulate"] for o, q in by[(kernel, d)] if o.op == C.OP_CHANNEL_SUM and o.shape == c.shape} == {0, 1} for c, _ in by[(kernel, d)]
                       if c.op == C.OP_CHANNEL_SUM)
        assert {(c.args["act"], r.two_pass) for c, r in by[(C.ACT_BWD_SUM, d)] + sums if c.op == C.OP_ACT_BWD_BIAS} == {(1, 0), (2, 0), (1, 1), (2, 1)}
        assert {r.path for _, r in by[(C.SUMSQ_ROWS, d)]} == {C.VECTOR, C.SCALAR}
        for kernel in (C.STDDEV_FWD, C.STDDEV_BWD, C.STDDEV_BWD_BWD):
            assert {r.E for _, r in by[(kernel, d)]} == {(4, 8)[d], 1} and {r.trips for _, r in by[(kernel, d)]} >= {1, 2}
            assert any(4 * c.shape[2] * c.shape[3] > 1024 for c, _ in by[(kernel, d)]) and any(c.args["sub"] == 2 for c, _ in by[(kernel, d)])


# (op, p, c, fy) -> route fields, by dtype where they differ: batch 8 on the pyramid 2x16 ... 128x1024 with 256, 256, 256, 256, 128, 64, 32 channels
def _pn(E, L, rows, grid, trips, nparts=0, levels=0, ws=0):
    return dict(kernel=C.PIXEL_NORM, E=E, P=1, U=2, L=L, rows=rows, grid_x=grid, trips=trips, nparts=nparts, levels=levels, ws_bytes=ws)


_MODEL = [
    ((C.OP_PN_FWD, 256, 256, 0), (_pn(4, 64, 1, 32, 1), _pn(8, 32, 2, 16, 1))),
    ((C.OP_PN_BWD_BIAS, 256, 256, 0), (_pn(4, 64, 1, 32, 1, 32, 1, 33 * 256 * 4), _pn(8, 32, 2, 16, 1, 16, 1, 17 * 256 * 4))),
    ((C.OP_PN_FWD, 16384, 256, 0), (_pn(4, 64, 1, 2048, 1), _pn(8, 32, 2, 1024, 1))),
    ((C.OP_PN_BWD_BIAS, 16384, 256, 0), (_pn(4, 64, 1, 1024, 2, 1024, 2, 1040 * 256 * 4), _pn(8, 32, 2, 1024, 1, 1024, 2, 1040 * 256 * 4))),
    ((C.OP_PN_FWD, 65536, 128, 0), (_pn(4, 32, 2, 4096, 1), _pn(8, 16, 4, 2048, 1))),
    ((C.OP_PN_BWD_BIAS, 65536, 128, 0), (_pn(4, 32, 2, 1024, 4, 1024, 2, 1040 * 128 * 4), _pn(8, 16, 4, 1024, 2, 1024, 2, 1040 * 128 * 4))),
    ((C.OP_PN_BWD_BWD, 262144, 64, 0), (_pn(4, 16, 4, 8192, 1), _pn(8, 8, 8, 4096, 1))),
    ((C.OP_PN_BWD_BIAS, 262144, 64, 0), (_pn(4, 16, 4, 1024, 8, 1024, 2, 1040 * 64 * 4), _pn(8, 8, 8, 1024, 4, 1024, 2, 1040 * 64 * 4))),
    ((C.OP_PN_BWD, 1048576, 32, 0), (_pn(4, 8, 8, 8192, 2), _pn(8, 4, 16, 8192, 1))),
    ((C.OP_PN_BWD_BIAS, 1048576, 32, 0), (_pn(4, 8, 8, 1024, 16, 1024, 2, 1040 * 32 * 4), _pn(8, 4, 16, 1024, 8, 1024, 2, 1040 * 32 * 4))),
    ((C.OP_CHANNEL_SUM, 256, 256, 0), dict(kernel=C.CHANNEL_SUM, path=C.QUADS, rows=4, grid_x=8, trips=8, nparts=8, levels=1, ws_bytes=9 * 256 * 4)),
    ((C.OP_ACT_BWD_BIAS, 256, 256, 0), dict(kernel=C.ACT_BWD_SUM, path=C.QUADS, rows=4, grid_x=8, nparts=8, levels=1, two_pass=0, ws_bytes=9 * 256 * 4)),
    ((C.OP_CHANNEL_SUM, 1048576, 32, 0), dict(kernel=C.CHANNEL_SUM, path=C.QUADS, rows=32, grid_x=2048, trips=16, nparts=2048, levels=2, ws_bytes=2080 * 32 * 4)),
    ((C.OP_ACT_BWD_BIAS, 1048576, 32, 0), dict(kernel=C.ACT_BWD_SUM, rows=32, grid_x=2048, nparts=2048, levels=2, two_pass=0)),
    ((C.OP_BIAS_ACT, 1048576, 32, 0), dict(kernel=C.BIAS_ACT, E=4, grid_x=8192, trips=4)),
    # the 2-channel images at 128x1024
    ((C.OP_BIAS_ACT, 1048576, 2, 0), dict(kernel=C.BIAS_ACT_SCALAR, E=1, grid_x=8192, trips=1)),
    ((C.OP_CHANNEL_SUM, 1048576, 2, 0), dict(kernel=C.CHANNEL_SUM, path=C.COLOUR, E=8, grid_x=1024, trips=1, nparts=1024, levels=2, ws_bytes=1040 * 2 * 4)),
    ((C.OP_ACT_BWD_BIAS, 1048576, 2, 0), dict(kernel=C.CHANNEL_SUM, path=C.COLOUR, two_pass=1, nparts=1024, levels=2)),
    ((C.OP_SUMSQ_ROWS, 262144, 0, 8), dict(kernel=C.SUMSQ_ROWS, path=C.VECTOR, grid_x=64, grid_y=8, per=1024, trips=4, tail=0, ws_bytes=8 * 64 * 4)),
    # the [batch][8192] bias sums of the dense layer
    ((C.OP_CHANNEL_SUM, 8, 8192, 0), dict(kernel=C.CHANNEL_SUM_ROWS, grid_x=32, trips=8, tail=0, nparts=0, levels=0, ws_bytes=2 * 8192 * 4)),
    ((C.OP_ACT_BWD_BIAS, 8, 8192, 0), dict(kernel=C.CHANNEL_SUM_ROWS, grid_x=32, two_pass=1, nparts=0, levels=0)),
    ((C.OP_CHANNEL_SUM, 16, 8192, 0), dict(kernel=C.CHANNEL_SUM_ROWS, grid_x=32, trips=16, nparts=0, levels=0)),
    # minibatch stddev on the 2x16x256 block, batch 8 and 4
    ((C.OP_STDDEV_FWD, 32, 256, 8), (dict(kernel=C.STDDEV_FWD, E=4, grid_x=2, trips=2, tail=0), dict(kernel=C.STDDEV_FWD, E=8, grid_x=2, trips=1, tail=0))),
    ((C.OP_STDDEV_BWD_BWD, 32, 256, 4), (dict(kernel=C.STDDEV_BWD_BWD, E=4, grid_x=1), dict(kernel=C.STDDEV_BWD_BWD, E=8, grid_x=1))),
]


def test_the_routes_of_the_model(lib):
    for (op, p, c, fy), want in _MODEL:
        for dtype in C.DTYPES:
            got = C.query(lib, op, dtype, p, c, fy)
            w = want[dtype] if isinstance(want, tuple) else want
            assert not isinstance(got, int) and {k: getattr(got, k) for k in w} == w, (C.OP_NAMES[op], p, c, dtype, got)


def test_query_refusals(lib):
    from gansynth_amd import _lib
    ints = (ctypes.c_int * _lib.EW_ROUTE_INTS)()
    q = lib.gs_elementwise_route
    assert q(C.OP_PN_FWD, C.BF16, 256, 32, 0, 0, -1, -1, ints) == 0
    assert q(18, C.BF16, 256, 32, 0, 0, -1, -1, ints) == -1 and b"op" in lib.gs_last_error()
    assert q(C.OP_PN_FWD, 2, 256, 32, 0, 0, -1, -1, ints) == -1 and b"dtype" in lib.gs_last_error()
    assert q(C.OP_PN_FWD, C.BF16, 256, 32, 0, 0, -1, -1, None) == -1
    assert q(C.OP_PN_FWD, C.BF16, 256, 32, 0, 0, 0, -1, ints) == -1 and q(C.OP_PN_FWD, C.BF16, 256, 32, 0, 0, -1, 0, ints) == -1 and b"cap" in lib.gs_last_error()
    # what the entry points refuse, with their code -- before anything is dereferenced or launched
    P = 0x10000
    for c in (2, 48, 2048):
        assert q(C.OP_PN_BWD, C.F32, 256, c, 0, 0, -1, -1, ints) == -1 and lib.gs_pixel_norm_fwd(P, P, 256, c, 1e-8, C.F32, None) == -1
        assert b"power of two" in lib.gs_last_error()
        assert lib.gs_pixel_norm_bwd_fused_bias(P, P, None, P, P, 256, c, 1e-8, 0, 0, 0, C.F32, P, 1 << 30, None) == -1 and b"power of two" in lib.gs_last_error()
    assert q(C.OP_ROW_SCALE, C.F32, 70, 0, 3, 0, -1, -1, ints) == -1 and lib.gs_row_scale(P, P, 1.0, P, 3, 70, C.F32, None) == -1 and b"multiple of 4" in lib.gs_last_error()
    assert q(C.OP_STDDEV_BWD, C.F32, 32, 16, 6, 0, -1, -1, ints) == -1 and lib.gs_batch_stddev_bwd(P, P, None, P, 6, 32, 16, 1e-8, C.F32, None) == -1
    assert b"multiple of 4" in lib.gs_last_error()
    assert lib.gs_channel_sum(P, P, 300, 32, 0, C.F32, P, 0, None) == -4 and b"workspace" in lib.gs_last_error()
    assert lib.gs_sumsq_rows(P, P, 3, 1027, C.F32, P, 0, None) == -4
    # rows > 1 with cols % 4 != 0 are not refused: they are read with scalar loads
    r = C.query(lib, C.OP_SUMSQ_ROWS, C.BF16, 1027, 0, 3)
    assert (r.path, r.E, r.per, r.tail) == (C.SCALAR, 1, 0, 1) and C.query(lib, C.OP_SUMSQ_ROWS, C.BF16, 1027, 0, 1).path == C.VECTOR


# ------------------------------------------------------------------------------------------------------------ the measure sees the errors
def _wrong(c, d, ref):
    """A float64 result with the error the case's family is there to catch, or None where the family has none to offer."""
    out = {k: v.clone() for k, v in ref.items()}
    if c.op in (C.OP_CHANNEL_SUM, C.OP_ACT_BWD_BIAS, C.OP_PN_BWD_BIAS):     # a sum missing its last row
        last = ref["gx"][-1] if "gx" in ref else d["g"].double()[-1]
        out["gb"] = ref["gb"] - last
    elif c.op == C.OP_BIAS_ACT and c.args["bias"]:                          # the bias shifted by one channel
        out = C.reference(c, dict(d, bias=torch.roll(d["bias"], 1)))
    elif c.op in (C.OP_ACT_BWD, C.OP_TANH_BWD_BWD, C.OP_AXPBY, C.OP_AXPBY_DEV, C.OP_ROW_SCALE, C.OP_UPSCALE, C.OP_BLOCKSUM, C.OP_SUMSQ_ROWS):   # the last element left at zero
        name = next(iter(out))
        out[name].view(-1)[-1] = 0.0
    elif c.op in (C.OP_PN_FWD, C.OP_PN_BWD, C.OP_PN_BWD_BWD):               # the last row group unnormalised
        rows = C.route_py(c.op, c.dtype, *C.words(c.op, c.shape, c.args)).rows
        src = {C.OP_PN_FWD: "x", C.OP_PN_BWD: "g", C.OP_PN_BWD_BWD: "gg"}[c.op]
        name = next(iter(out))
        out[name][-rows:] = d[src].double()[-rows:]
    elif c.op in STDDEV_OPS:                                                # the last member's statistic / gradient missing
        for v in out.values():
            v[-1] = 0.0
    else:
        return None
    return out



def test_the_measure_sees_a_wrong_row_channel_or_element():
    seen = set()
    for c in C.CASES:
        d = C.inputs(c)
        ref = C.reference(c, d)
        out_dtype = {name: (torch.float32 if name == "gb" or c.op == C.OP_SUMSQ_ROWS else C.TORCH_DTYPE[c.dtype]) for name in ref}
        for name, v in ref.items():   # the right result, rounded as the kernel stores it, passes
            r, ok = C.within(c, name, v.to(out_dtype[name]), v)
            assert ok, (C.case_id(c), name, r)
        bad = _wrong(c, d, ref)
        if bad is None:
            continue
        caught = [name for name, v in bad.items() if not C.within(c, name, v.to(out_dtype[name]), ref[name])[1]]
        # (a row of 512 or 1024 unit-variance channels has an rms within a fraction of a percent of 1: left unnormalised it IS nearly right, and
        #  one bf16 rounding hides it -- the narrow rows of the same kernel do not)
        assert caught or (c.op in (C.OP_PN_FWD, C.OP_PN_BWD, C.OP_PN_BWD_BWD) and c.shape[1] >= 256), C.case_id(c)
        if caught:
            seen.add((c.op, c.dtype))
    assert seen == set(itertools.product(range(18), C.DTYPES))
