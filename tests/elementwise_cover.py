"""The cases of the elementwise / row-reduction kernels (csrc/elementwise.hip) and the batch-stddev kernels (csrc/small_ops.hip) -- shared by
tests/test_elementwise_cover_cpu.py and tests/test_elementwise_cover_gpu.py (a plain helper module: no fixtures, no collection hooks).

KERNELS is the list of compiled instantiations as the launchers spell them; a case is an operation, a dtype, a shape and what is asked of it
(activation, bias, accumulate, addend ...), together with the instantiation `key` it is there for and `want`: the route fields that make it the
case it claims to be (path, tail, levels, trips ...).  Which kernel a case runs is not decided here: both test files ask the library
(gs_elementwise_route, host arithmetic on the route the entry points read) and hold the answer against the case.  `route_py` is a restatement of
csrc/elementwise_route.h for the CPU test's sweep.  `reference` is float64 on the operands as stored (activations rounded to bf16 for bf16),
written from the definition of each operation: the norm and stddev gradients are torch.autograd.grad of the float64 forward, the fused forms are
composed around them, sums are float64 sums.
"""
import ctypes
from collections import namedtuple

import torch

from tests import igemm_cover

F32, BF16 = 0, 1
DTYPES = (F32, BF16)
DTYPE_NAMES = ("f32", "bf16")
TORCH_DTYPE = {F32: torch.float32, BF16: torch.bfloat16}
NONE, LRELU, TANH = 0, 1, 2                                            # GS_ACT_*
ACT_NAMES = ("none", "lrelu", "tanh")
ERR_ARG = -1
EPS = 1.0e-12   # pixel_normalization / batch_stddev of the model (gansynth_amd/ops.py)
(OP_BIAS_ACT, OP_ACT_BWD, OP_TANH_BWD_BWD, OP_AXPBY, OP_AXPBY_DEV, OP_UPSCALE, OP_ROW_SCALE, OP_CHANNEL_SUM, OP_ACT_BWD_BIAS, OP_PN_FWD, OP_PN_BWD,
 OP_PN_BWD_BIAS, OP_PN_BWD_BWD, OP_BLOCKSUM, OP_SUMSQ_ROWS, OP_STDDEV_FWD, OP_STDDEV_BWD, OP_STDDEV_BWD_BWD) = range(18)   # GS_EW_OP_*
OP_NAMES = ("bias_act", "act_bwd", "tanh_bwd_bwd", "axpby", "axpby_dev", "upscale", "row_scale", "channel_sum", "act_bwd_bias", "pixel_norm_fwd",
            "pixel_norm_bwd", "pixel_norm_bwd_bias", "pixel_norm_bwd_bwd", "blocksum", "sumsq_rows", "batch_stddev_fwd", "batch_stddev_bwd",
            "batch_stddev_bwd_bwd")
(BIAS_ACT, BIAS_ACT_SCALAR, ACT_BWD, TANH_BWD_BWD, AXPBY, AXPBY_DEV, UPSCALE, ROW_SCALE, CHANNEL_SUM, CHANNEL_SUM_ROWS, ACT_BWD_SUM, PIXEL_NORM, BLOCKSUM,
 BLOCKSUM_SMALL, SUMSQ_ROWS, STDDEV_FWD, STDDEV_BWD, STDDEV_BWD_BWD) = range(18)   # GS_EW_*
KERNEL_NAMES = ("bias_act", "bias_act_scalar", "act_bwd", "tanh_bwd_bwd", "axpby", "axpby_dev", "upscale", "row_scale", "channel_sum", "channel_sum_rows",
                "act_bwd_sum", "pixel_norm", "blocksum", "blocksum_small", "sumsq_rows", "batch_stddev_fwd", "batch_stddev_bwd", "batch_stddev_bwd_bwd")
PATH_NONE, COLOUR, QUADS, GENERIC, VECTOR, SCALAR = range(6)           # GS_EW_PATH_*
ROUTE_FIELDS = ("kernel", "path", "E", "P", "U", "L", "rows", "grid_x", "grid_y", "trips", "tail", "nparts", "levels", "per", "two_pass", "reserved", "ws_bytes")
CS_SLAB, SSQ_CHUNKS, EW_CAP, PN_BIAS_CAP = 64, 64, 8192, 1024
KNOBS = {"GS_EW_GRID_CAP": "2", "GS_PN_BIAS_GRID_CAP": "2"}   # the child of the GPU test: every grid-stride loop takes several trips
GRID_STRIDE = (BIAS_ACT, BIAS_ACT_SCALAR, ACT_BWD, TANH_BWD_BWD, AXPBY, AXPBY_DEV, UPSCALE, ROW_SCALE, PIXEL_NORM, BLOCKSUM, BLOCKSUM_SMALL)

# Ceilings of max |ref| for an fp32 result, those of the suite's own tests of these kernels (tests/test_kernels_gpu.py): forward, streaming and sums;
# first- and second-order norm and stddev gradients; axpby and row_scale.  A bf16 result is computed in fp32 and rounded once, to nearest even, on
# the store: element by element |got - ref| <= 2^-8 |ref| + ceiling * max |ref| (one rounding, 2^-9 of the value, with a factor 2 of margin).
CEIL_FWD, CEIL_GRAD, CEIL_AXPBY = 1e-5, 1e-4, 1e-6
_GRAD_OPS = (OP_PN_BWD, OP_PN_BWD_BIAS, OP_PN_BWD_BWD, OP_STDDEV_BWD, OP_STDDEV_BWD_BWD)


def ceiling(op, name):
    if op in (OP_AXPBY, OP_AXPBY_DEV, OP_ROW_SCALE):
        return CEIL_AXPBY
    return CEIL_GRAD if op in _GRAD_OPS and name != "gb" else CEIL_FWD   # (gb: a sum)


Key = namedtuple("Key", "kernel dtype params")   # one compiled instantiation; params: the template arguments behind the dtype
Route = namedtuple("Route", ROUTE_FIELDS)
# shape: by op (words()); args: what is asked; want: route fields (and facts()) the case is there for
Case = namedtuple("Case", "op dtype shape args key want")


def _key(kernel, dtype, *params):
    return Key(kernel, dtype, tuple(params))


def _pn_pairs(d):
    """(E, P, U) of the pixel-norm instantiations: fp32 E = 4; bf16 E = 8 and, for rows of 4 channels, E = 4."""
    return ((4, 1, 2), (4, 2, 1), (4, 4, 1)) if d == F32 else ((8, 1, 2), (8, 2, 1), (4, 1, 2))


KERNELS = (
    [_key(BIAS_ACT, d, act, bias) for d in DTYPES for act in (0, 1, 2) for bias in (1, 0)]
    + [_key(k, d) for d in DTYPES for k in (BIAS_ACT_SCALAR, TANH_BWD_BWD, AXPBY, AXPBY_DEV, UPSCALE, ROW_SCALE, BLOCKSUM, BLOCKSUM_SMALL, SUMSQ_ROWS)]
    + [_key(k, d, act) for d in DTYPES for k in (ACT_BWD, ACT_BWD_SUM) for act in (1, 2)]
    + [_key(k, d, act) for d in DTYPES for k in (CHANNEL_SUM, CHANNEL_SUM_ROWS) for act in (0, 1, 2)]   # act != 0: the sums of the two-pass act_bwd_bias
    + [_key(PIXEL_NORM, d, mode, E, P, U, bs) for d in DTYPES for mode, bs in ((0, 0), (1, 0), (1, 1), (2, 0)) for E, P, U in _pn_pairs(d)]
    + [_key(k, d, vn) for d in DTYPES for k in (STDDEV_FWD, STDDEV_BWD, STDDEV_BWD_BWD) for vn in ((4, 8)[d], 1)]
)
assert len(KERNELS) == len(set(KERNELS)) == 86


def key_id(k):
    return "-".join([KERNEL_NAMES[k.kernel], DTYPE_NAMES[k.dtype]] + [str(v) for v in k.params])


def case_id(c):
    args = "+".join(f"{k}={v}" for k, v in sorted(c.args.items()))
    return f"{OP_NAMES[c.op]}-{DTYPE_NAMES[c.dtype]} {'x'.join(str(v) for v in c.shape)} {args}".rstrip()


def words(op, shape, args):
    """(p, c, fy, fx) of gs_elementwise_route for a case's shape."""
    if op in (OP_BIAS_ACT, OP_CHANNEL_SUM, OP_ACT_BWD_BIAS, OP_PN_FWD, OP_PN_BWD, OP_PN_BWD_BIAS, OP_PN_BWD_BWD):
        return shape[0], shape[1], 0, 0
    if op in (OP_ACT_BWD, OP_TANH_BWD_BWD, OP_AXPBY, OP_AXPBY_DEV):
        return shape[0], 0, 0, 0
    if op == OP_UPSCALE:     # shape: the INPUT (n, c, h, w)
        n, c, h, w = shape
        return n * h * args["fy"] * w * args["fx"] * c, c, args["fy"], args["fx"]
    if op == OP_BLOCKSUM:    # shape: the OUTPUT (n, c, ho, wo)
        n, c, h, w = shape
        return n * h * w * c, c, args["fy"], args["fx"]
    if op in (OP_ROW_SCALE, OP_SUMSQ_ROWS):
        return shape[1], 0, shape[0], 0
    b, c, h, w = shape       # stddev: one call per sub-batch
    return h * w, c, b // args.get("sub", 1), 0


def query(lib, op, dtype, p, c, fy=0, fx=0, ew_cap=-1, pn_cap=-1):
    """gs_elementwise_route: a Route, or the negative code the entry point refuses the call with.  Caps -1: this process's environment."""
    from gansynth_amd import _lib
    ints = (ctypes.c_int * _lib.EW_ROUTE_INTS)()
    rc = lib.gs_elementwise_route(op, dtype, p, c, fy, fx, ew_cap, pn_cap, ints)
    return rc if rc else Route(*ints[:16], (ints[16] & 0xFFFFFFFF) | (ints[17] << 32))


def route(lib, c, ew_cap=-1, pn_cap=-1):
    return query(lib, c.op, c.dtype, *words(c.op, c.shape, c.args), ew_cap=ew_cap, pn_cap=pn_cap)


def route_keys(op, dtype, r, args):
    """The instantiations a routed call launches, from the route and what the call asks (activation, bias): its own kernel and, for the
    two-pass act_bwd_bias (whose channel sum is the ACT instantiation), the act_bwd launch behind it."""
    k = r.kernel
    if k == BIAS_ACT:
        keys = {_key(k, dtype, args.get("act", 0), int(bool(args.get("bias", 0))))}
    elif k in (ACT_BWD, ACT_BWD_SUM):
        keys = {_key(k, dtype, args["act"])}
    elif k == PIXEL_NORM:
        mode = {OP_PN_FWD: 0, OP_PN_BWD: 1, OP_PN_BWD_BIAS: 1, OP_PN_BWD_BWD: 2}[op]
        keys = {_key(k, dtype, mode, r.E, r.P, r.U, int(op == OP_PN_BWD_BIAS))}
    elif k in (STDDEV_FWD, STDDEV_BWD, STDDEV_BWD_BWD):
        keys = {_key(k, dtype, r.E)}
    elif k in (CHANNEL_SUM, CHANNEL_SUM_ROWS):
        keys = {_key(k, dtype, args["act"] if r.two_pass else 0)}
    else:
        keys = {_key(k, dtype)}
    if r.two_pass:
        keys.add(_key(ACT_BWD, dtype, args["act"]))
    return keys


def facts(c, r):
    """What a route means for its case, beyond the fields: the derived properties `want` may name."""
    p = words(c.op, c.shape, c.args)[0]
    f = r._asdict()
    f["ragged_slab"] = int(r.levels == 2 and r.nparts % CS_SLAB != 0)
    if r.kernel in (CHANNEL_SUM, ACT_BWD_SUM) and r.rows:
        step, per = r.nparts * r.rows, (4 if r.kernel == CHANNEL_SUM else 2)
        f["unrolled_trip"] = int(p > (per - 1) * step)           # row lane 0 of block 0 makes a trip of the unrolled loop
        f["single_rows"] = int(p % (per * step) != 0)            # ... and somebody a single-row tail trip
        f["idle_threads"] = 256 - r.rows * min(c.shape[1] // 4 if r.path == QUADS else c.shape[1], 256)
        f["channel_trips"] = -(-c.shape[1] // 256) if r.path == GENERIC else 1
    if r.kernel == PIXEL_NORM:
        f["partial_last_trip"] = int(p % (r.grid_x * 4 * r.rows * r.U) != 0)
        f["ragged_wave"] = int(p % r.rows != 0)
    if r.kernel == SUMSQ_ROWS:
        f["empty_chunks"] = int(r.per * (SSQ_CHUNKS - 1) >= max(p >> 2, 1)) if r.path == VECTOR else 0
    return f


# ------------------------------------------------------------------------------------------------------------- the route, restated
def _cdiv(a, b):
    return -(-a // b)


def _grid(nvec, cap):
    return max(1, min(_cdiv(nvec, 256), cap))


def _parts(p, c):
    rpb = max(1, 256 // ((c // 4 if c % 4 == 0 else min(c, 256)) if c >= 4 else c))
    return max(1, min(_cdiv(p, rpb * 8), 2048))


def _route(**kw):
    d = dict.fromkeys(ROUTE_FIELDS, 0)
    d.update(kw)
    return Route(**d)


def _partials(nparts, c):
    return dict(nparts=nparts, levels=1 if nparts <= CS_SLAB else 2, ws_bytes=(nparts + _cdiv(nparts, CS_SLAB)) * c * 4)


def _channel_sum_py(p, c, **extra):
    np_ = _parts(p, c)
    part = _partials(np_, c)
    if p <= 64 and c >= 256:
        return _route(kernel=CHANNEL_SUM_ROWS, E=1, grid_x=_cdiv(c, 256), grid_y=1, trips=p, tail=int(c % 256 != 0), ws_bytes=part["ws_bytes"], **extra)
    if c in (1, 2, 4) and (p * c) % 8 == 0:
        return _route(kernel=CHANNEL_SUM, path=COLOUR, E=8, grid_x=np_, grid_y=1, trips=_cdiv(p * c // 8, np_ * 256), **part, **extra)
    if c % 4 == 0 and c <= 1024:
        rows = max(256 // (c // 4), 1)
        return _route(kernel=CHANNEL_SUM, path=QUADS, E=4, rows=rows, grid_x=np_, grid_y=1, trips=_cdiv(p, np_ * rows), **part, **extra)
    rows = 256 // min(c, 256)
    return _route(kernel=CHANNEL_SUM, path=GENERIC, E=1, rows=rows, grid_x=np_, grid_y=1, trips=_cdiv(p, np_ * rows), **part, **extra)


def route_py(op, dtype, p, c, fy=0, fx=0, ew_cap=EW_CAP, pn_cap=PN_BIAS_CAP):
    """csrc/elementwise_route.h: elementwise_route, condition for condition: a Route or the error code."""
    wn = 4 if dtype == F32 else 8

    def stream(kernel, E, n):
        g = _grid((n >> 2) + 4 if E == 4 else n, ew_cap)
        return _route(kernel=kernel, E=E, grid_x=g, grid_y=1, trips=_cdiv(n >> 2 if E == 4 else n, g * 256), tail=int(E == 4 and n % 4 != 0))
    if dtype not in DTYPES:
        return ERR_ARG
    if op == OP_BIAS_ACT:
        if not (p > 0 and c > 0):
            return ERR_ARG
        n = p * c // 4 if c % 4 == 0 else p * c
        g = _grid(n, ew_cap)
        return _route(kernel=BIAS_ACT if c % 4 == 0 else BIAS_ACT_SCALAR, E=4 if c % 4 == 0 else 1, grid_x=g, grid_y=1, trips=_cdiv(n, g * 256))
    if op in (OP_ACT_BWD, OP_AXPBY, OP_AXPBY_DEV, OP_TANH_BWD_BWD):
        if p <= 0:
            return ERR_ARG
        return stream({OP_ACT_BWD: ACT_BWD, OP_AXPBY: AXPBY, OP_AXPBY_DEV: AXPBY_DEV, OP_TANH_BWD_BWD: TANH_BWD_BWD}[op], 1 if op == OP_TANH_BWD_BWD else 4, p)
    if op == OP_UPSCALE:
        return stream(UPSCALE, 1, p) if p > 0 and fy > 0 and fx > 0 else ERR_ARG
    if op == OP_ROW_SCALE:
        if not (fy > 0 and p > 0 and p % 4 == 0):
            return ERR_ARG
        g = _grid(fy * p // 4, ew_cap)
        return _route(kernel=ROW_SCALE, E=4, grid_x=g, grid_y=1, trips=_cdiv(fy * p // 4, g * 256))
    if op == OP_CHANNEL_SUM:
        return _channel_sum_py(p, c) if p > 0 and c > 0 else ERR_ARG
    if op == OP_ACT_BWD_BIAS:
        if not (p > 0 and c > 0):
            return ERR_ARG
        if c % 4 != 0 or c > 1024 or 256 % (c // 4) != 0:
            return _channel_sum_py(p, c, two_pass=1)
        np_, rows = _parts(p, c), 256 // (c // 4)
        return _route(kernel=ACT_BWD_SUM, path=QUADS, E=4, rows=rows, grid_x=np_, grid_y=1, trips=_cdiv(p, np_ * rows), **_partials(np_, c))
    if op in (OP_PN_FWD, OP_PN_BWD, OP_PN_BWD_BIAS, OP_PN_BWD_BWD):
        if not (p > 0 and 4 <= c <= 1024 and c & (c - 1) == 0):
            return ERR_ARG
        E = wn if c % wn == 0 else 4
        L = min(c // E, 64)
        P = c // E // L
        U = 2 if P == 1 else 1
        rpb = 4 * (64 // L) * U
        g = _grid(_cdiv(p, rpb) * 256, ew_cap)
        part = {}
        if op == OP_PN_BWD_BIAS:
            g = min(g, pn_cap)
            part = _partials(g, c)
        return _route(kernel=PIXEL_NORM, E=E, P=P, U=U, L=L, rows=64 // L, grid_x=g, grid_y=1, trips=_cdiv(p, g * rpb), **part)
    if op == OP_BLOCKSUM:
        if not (p > 0 and fy > 0 and fx > 0):
            return ERR_ARG
        if fy * fx >= 32:
            g = _grid(p * 64, ew_cap)
            return _route(kernel=BLOCKSUM, E=1, grid_x=g, grid_y=1, trips=_cdiv(p, g * 4), tail=int(fy * fx % 64 != 0))
        g = _grid(p, ew_cap)
        return _route(kernel=BLOCKSUM_SMALL, E=1, grid_x=g, grid_y=1, trips=_cdiv(p, g * 256))
    if op == OP_SUMSQ_ROWS:
        if not (fy > 0 and p > 0):
            return ERR_ARG
        vec = p % 4 == 0 or fy == 1
        nvec = p // 4 if vec else 0
        per = _cdiv(nvec, SSQ_CHUNKS)
        return _route(kernel=SUMSQ_ROWS, path=VECTOR if vec else SCALAR, E=4 if vec else 1, grid_x=SSQ_CHUNKS, grid_y=fy, per=per,
                      trips=_cdiv(per, 256) if vec else _cdiv(p, 256), tail=int(nvec * 4 != p), ws_bytes=fy * SSQ_CHUNKS * 4)
    if op in (OP_STDDEV_FWD, OP_STDDEV_BWD, OP_STDDEV_BWD_BWD):
        if not (fy > 0 and fy % 4 == 0 and p > 0 and c > 0):
            return ERR_ARG
        vn = wn if p * c % wn == 0 else 1
        return _route(kernel={OP_STDDEV_FWD: STDDEV_FWD, OP_STDDEV_BWD: STDDEV_BWD, OP_STDDEV_BWD_BWD: STDDEV_BWD_BWD}[op], E=vn, grid_x=fy // 4, grid_y=1,
                      trips=_cdiv(p * c, 1024 * vn), tail=int(p * c % (1024 * vn) != 0))
    return ERR_ARG


# ---------------------------------------------------------------------------------------------------------------------------------- the cases
PN_WIDTHS = (4, 8, 16, 32, 64, 128, 256, 512, 1024)


def pn_rows(dtype, c):
    """Rows for a pixel-norm case: three blocks (two under the knobs, which then take two trips), a ragged last wave, and a last trip in
    which an unrolled row group is out of range."""
    r = route_py(OP_PN_FWD, dtype, 1, c)
    rpb = 4 * r.rows * r.U
    return 2 * rpb + r.rows + (1 if r.rows > 1 else 0)


def _cases():
    out = []

    def add(op, d, shape, key, want=None, **args):
        out.append(Case(op, d, tuple(shape), args, _key(key[0], d, *key[1:]), want or {}))
    for d in DTYPES:
        wn = (4, 8)[d]
        # ---- bias + activation: vector (c % 4 == 0), scalar (the 2-channel images; 61 logits); 2 trips under the knob
        for act in (NONE, LRELU, TANH):
            for bias in (1, 0):
                add(OP_BIAS_ACT, d, (37, 8), (BIAS_ACT, act, bias), act=act, bias=bias)
                add(OP_BIAS_ACT, d, (37, 2), (BIAS_ACT_SCALAR,), act=act, bias=bias)
                add(OP_BIAS_ACT, d, (5, 61), (BIAS_ACT_SCALAR,), act=act, bias=bias)
        add(OP_BIAS_ACT, d, (300, 8), (BIAS_ACT, LRELU, 1), act=LRELU, bias=1)
        add(OP_BIAS_ACT, d, (700, 2), (BIAS_ACT_SCALAR,), act=TANH, bias=1)
        # ---- streaming kernels with a sub-vector tail: tail only, vectors only, both; 4099: 2 trips under the knob
        for n in (3, 1024, 1027, 4099):
            tail = {"tail": int(n % 4 != 0)}
            for act in (LRELU, TANH):
                add(OP_ACT_BWD, d, (n,), (ACT_BWD, act), tail, act=act)
            add(OP_TANH_BWD_BWD, d, (n,), (TANH_BWD_BWD,))
            add(OP_AXPBY, d, (n,), (AXPBY,), tail)
            add(OP_AXPBY_DEV, d, (n,), (AXPBY_DEV,), tail)
        for alpha in (1.0, 2.0):
            add(OP_ROW_SCALE, d, (3, 20), (ROW_SCALE,), alpha=alpha)
        add(OP_ROW_SCALE, d, (3, 700), (ROW_SCALE,), alpha=2.0)
        # ---- upscale: the index map, bit-exact at scale 1
        add(OP_UPSCALE, d, (1, 4, 4, 4), (UPSCALE,), fy=3, fx=2, scale=1.0)
        add(OP_UPSCALE, d, (2, 2, 2, 16), (UPSCALE,), fy=2, fx=2, scale=1.0)
        add(OP_UPSCALE, d, (2, 2, 4, 16), (UPSCALE,), fy=2, fx=2, scale=0.5)
        # ---- channel sums, every path with accumulate off and on
        for acc in (0, 1):
            add(OP_CHANNEL_SUM, d, (64, 256), (CHANNEL_SUM_ROWS, 0), {"tail": 0, "levels": 0}, accumulate=acc)
            add(OP_CHANNEL_SUM, d, (5, 300), (CHANNEL_SUM_ROWS, 0), {"tail": 1, "levels": 0, "grid_x": 2}, accumulate=acc)   # ragged last block
            for c, p in ((1, 80), (2, 76), (4, 78)):
                add(OP_CHANNEL_SUM, d, (p, c), (CHANNEL_SUM, 0), {"path": COLOUR}, accumulate=acc)
            add(OP_CHANNEL_SUM, d, (77, 4), (CHANNEL_SUM, 0), {"path": QUADS, "rows": 256}, accumulate=acc)          # c = 4 off the colour branch
            add(OP_CHANNEL_SUM, d, (700, 12), (CHANNEL_SUM, 0), {"path": QUADS, "rows": 85, "idle_threads": 1}, accumulate=acc)
            add(OP_CHANNEL_SUM, d, (70, 1024), (CHANNEL_SUM, 0), {"path": QUADS, "rows": 1, "idle_threads": 0}, accumulate=acc)   # quads = 256
            add(OP_CHANNEL_SUM, d, (1500, 32), (CHANNEL_SUM, 0), {"path": QUADS, "unrolled_trip": 1, "single_rows": 1}, accumulate=acc)
            add(OP_CHANNEL_SUM, d, (77, 2), (CHANNEL_SUM, 0), {"path": GENERIC}, accumulate=acc)                    # c = 2 off the colour branch
            add(OP_CHANNEL_SUM, d, (300, 61), (CHANNEL_SUM, 0), {"path": GENERIC, "rows": 4}, accumulate=acc)
            add(OP_CHANNEL_SUM, d, (70, 261), (CHANNEL_SUM, 0), {"path": GENERIC, "channel_trips": 2}, accumulate=acc)   # the c0 loop
            add(OP_CHANNEL_SUM, d, (70, 1028), (CHANNEL_SUM, 0), {"path": GENERIC, "channel_trips": 5}, accumulate=acc)
            add(OP_CHANNEL_SUM, d, (16700, 32), (CHANNEL_SUM, 0), {"path": QUADS, "nparts": 66, "levels": 2, "ragged_slab": 1}, accumulate=acc)
        # ---- activation backward with the bias sums: one pass (two-row trips and a single-row tail), two passes
        for act, acc in ((LRELU, 0), (TANH, 1)):
            for c, p in ((4, 800), (32, 100), (1024, 3)):
                add(OP_ACT_BWD_BIAS, d, (p, c), (ACT_BWD_SUM, act), {"two_pass": 0, "unrolled_trip": 1, "single_rows": 1}, act=act, accumulate=acc)
            for (p, c), path in (((77, 2), GENERIC), ((76, 2), COLOUR), ((77, 12), QUADS), ((77, 61), GENERIC)):
                add(OP_ACT_BWD_BIAS, d, (p, c), (CHANNEL_SUM, act), {"two_pass": 1, "path": path}, act=act, accumulate=acc)
            for p, c in ((5, 300), (8, 8192)):   # few rows, many channels: a thread per channel (the dense layer's [batch][8192])
                add(OP_ACT_BWD_BIAS, d, (p, c), (CHANNEL_SUM_ROWS, act), {"two_pass": 1, "levels": 0}, act=act, accumulate=acc)
        # ---- pixel norm: every reachable (E, P, L), the four entry points at each
        for c in PN_WIDTHS:
            p = pn_rows(d, c)
            r = route_py(OP_PN_FWD, d, p, c)
            epu = (r.E, r.P, r.U)
            want = {"L": r.L, "partial_last_trip": 1, "ragged_wave": int(r.rows > 1)}
            add(OP_PN_FWD, d, (p, c), (PIXEL_NORM, 0) + epu + (0,), want)
            add(OP_PN_BWD, d, (p, c), (PIXEL_NORM, 1) + epu + (0,), want, pre=LRELU, post=LRELU, addend=1)
            for acc in (0, 1):
                add(OP_PN_BWD_BIAS, d, (p, c), (PIXEL_NORM, 1) + epu + (1,), want, pre=LRELU, post=LRELU, addend=1, accumulate=acc)
            add(OP_PN_BWD_BWD, d, (p, c), (PIXEL_NORM, 2) + epu + (0,), want, pre=LRELU, out2=1)
            if c != 32:
                continue
            for pre in (NONE, LRELU, TANH):   # every fused form once
                for post in (NONE, LRELU, TANH):
                    for addend in (0, 1):
                        if (pre, post, addend) != (LRELU, LRELU, 1):
                            add(OP_PN_BWD, d, (p, c), (PIXEL_NORM, 1) + epu + (0,), want, pre=pre, post=post, addend=addend)
                            add(OP_PN_BWD_BIAS, d, (p, c), (PIXEL_NORM, 1) + epu + (1,), want, pre=pre, post=post, addend=addend, accumulate=(pre + post + addend) % 2)
                for out2 in (0, 1):
                    if (pre, out2) != (LRELU, 1):
                        add(OP_PN_BWD_BWD, d, (p, c), (PIXEL_NORM, 2) + epu + (0,), want, pre=pre, out2=out2)
        # ---- block sums: a thread per output (fy * fx < 32), a wave per output (whole and partial 64-element trips)
        for fy, fx in ((2, 2), (3, 2), (1, 1)):
            for scale in sorted({1.0, 1.0 / (fy * fx)}):
                add(OP_BLOCKSUM, d, (2, 2, 2, 16), (BLOCKSUM_SMALL,), fy=fy, fx=fx, scale=scale)
        add(OP_BLOCKSUM, d, (2, 2, 8, 40), (BLOCKSUM_SMALL,), fy=2, fx=2, scale=0.25)
        for (fy, fx), tail in (((4, 8), 1), ((5, 7), 1), ((9, 9), 1), ((64, 64), 0)):
            for scale in (1.0, 1.0 / (fy * fx)):
                add(OP_BLOCKSUM, d, (2, 2, 2, 16), (BLOCKSUM,), {"tail": tail}, fy=fy, fx=fx, scale=scale)
        # ---- sums of squares per row: most chunks empty; several trips per chunk; the sub-vector tail; rows off the 4-element alignment
        add(OP_SUMSQ_ROWS, d, (3, 8), (SUMSQ_ROWS,), {"path": VECTOR, "empty_chunks": 1, "tail": 0})
        add(OP_SUMSQ_ROWS, d, (2, 70000), (SUMSQ_ROWS,), {"path": VECTOR, "trips": 2, "tail": 0})
        add(OP_SUMSQ_ROWS, d, (1, 70003), (SUMSQ_ROWS,), {"path": VECTOR, "trips": 2, "tail": 1})
        add(OP_SUMSQ_ROWS, d, (3, 1027), (SUMSQ_ROWS,), {"path": SCALAR, "per": 0, "tail": 1, "trips": 5})
        # ---- batch stddev, all orders: wide with two trips, wide with one partial trip, scalar, 4 hw > 1024, two sub-batches
        shapes = [((8, 256, 2, 16) if d == F32 else (4, 256, 4, 16), wn, {"trips": 2, "tail": 0}, 1), ((8, 16, 3, 5), wn, {"trips": 1, "tail": 1}, 1),
                  ((8, 3, 3, 5), 1, {}, 1), ((4, 4, 10, 30), wn, {}, 1), ((8, 16, 3, 5), wn, {}, 2)]
        if d == BF16:
            shapes.append(((4, 4, 1, 5), 1, {}, 1))   # hw * c a multiple of 4, not of 8
        for shape, vn, want, sub in shapes:
            add(OP_STDDEV_FWD, d, shape, (STDDEV_FWD, vn), want, sub=sub)
            for addend in (0, 1):
                add(OP_STDDEV_BWD, d, shape, (STDDEV_BWD, vn), want, addend=addend, sub=sub)
            add(OP_STDDEV_BWD_BWD, d, shape, (STDDEV_BWD_BWD, vn), want, sub=sub)
    return out


CASES = _cases()


def families():
    """(kernel template, dtype) of every GPU test, with its cases (a two-pass act_bwd_bias case rides with both of its kernels)."""
    out = {}
    for c in CASES:
        r = route_py(c.op, c.dtype, *words(c.op, c.shape, c.args))
        for k in route_keys(c.op, c.dtype, r, c.args):
            out.setdefault((k.kernel, k.dtype), []).append(c)
    return out


def family_id(f):
    return f"{KERNEL_NAMES[f[0]]}-{DTYPE_NAMES[f[1]]}"


# --------------------------------------------------------------------------------------------------------------------- operands and reference
def _lrelu(t):
    return torch.where(t > 0, t, 0.2 * t)


def _act_out(t, act):
    """A tensor that stands for the OUTPUT of an activation: no exact zeros behind leaky_relu, inside (-1, 1) behind tanh."""
    return torch.tanh(t) if act == TANH else (_lrelu(t) if act == LRELU else t)


def _dact(x, act):
    """act' through the activation output x (float64)."""
    return torch.where(x > 0, 1.0, 0.2).to(x.dtype) if act == LRELU else (1.0 - x * x if act == TANH else torch.ones_like(x))


def inputs(c, seed=7):
    """The operands of a case as stored (CPU; activations rounded to the case's dtype, fp32 accumulators and bias as they are)."""
    g = torch.Generator().manual_seed(seed)
    dt = TORCH_DTYPE[c.dtype]
    a = c.args

    def rn(*shape):
        return torch.randn(*shape, generator=g)
    d = {}
    if c.op == OP_BIAS_ACT:
        d["x"] = rn(*c.shape).to(dt)
        if a["bias"]:
            d["bias"] = rn(c.shape[1])
    elif c.op in (OP_ACT_BWD, OP_TANH_BWD_BWD):
        d["y"] = _act_out(rn(*c.shape), a.get("act", TANH)).to(dt)
        d["g"], d["gg"] = rn(*c.shape).to(dt), rn(*c.shape).to(dt)
    elif c.op in (OP_AXPBY, OP_AXPBY_DEV):
        d["a"], d["b"] = rn(*c.shape).to(dt), rn(*c.shape).to(dt)
        d["ca"] = torch.tensor(0.3, dtype=torch.float32)          # as the kernel receives them: fp32
        d["cb"] = torch.tensor(1.0 - 0.3, dtype=torch.float32)
    elif c.op == OP_ROW_SCALE:
        d["x"], d["s"] = rn(*c.shape).to(dt), rn(c.shape[0])
    elif c.op == OP_UPSCALE:
        d["x"] = rn(*c.shape).to(dt)
    elif c.op == OP_BLOCKSUM:
        n, ch, h, w = c.shape
        d["x"] = rn(n, ch, h * a["fy"], w * a["fx"]).to(dt)
    elif c.op == OP_CHANNEL_SUM:
        d["g"] = rn(*c.shape).to(dt)
    elif c.op == OP_ACT_BWD_BIAS:
        d["y"], d["g"] = _act_out(rn(*c.shape), a["act"]).to(dt), rn(*c.shape).to(dt)
    elif c.op in (OP_PN_FWD, OP_PN_BWD, OP_PN_BWD_BIAS, OP_PN_BWD_BWD):
        kind = TANH if TANH in (a.get("pre"), a.get("post")) else (LRELU if LRELU in (a.get("pre"), a.get("post")) else NONE)
        d["x"] = _act_out(rn(*c.shape), kind).to(dt)
        d["g"], d["gg"], d["addend"] = rn(*c.shape).to(dt), rn(*c.shape).to(dt), rn(*c.shape).to(dt)
    elif c.op == OP_SUMSQ_ROWS:
        d["x"] = rn(*c.shape).to(dt)
    else:
        b, ch, h, w = c.shape
        d["x"], d["gy"], d["ggx"], d["addend"] = rn(b, ch, h, w).to(dt), rn(b, 1, h, w).to(dt), rn(b, ch, h, w).to(dt), rn(b, ch, h, w).to(dt)
    if a.get("accumulate"):
        d["acc0"] = 0.5 * rn(c.shape[1]) + 0.25   # a non-zero fp32 buffer
    if c.op in (OP_ACT_BWD_BIAS, OP_PN_BWD, OP_PN_BWD_BIAS, OP_PN_BWD_BWD) or c.op == OP_ACT_BWD and a["act"] == LRELU:
        key = "x" if "x" in d else "y"
        assert not bool((d[key].float() == 0).any()), "an activation output that a sign is read from has no exact zeros"
    return d


def _pixel_norm64(x):
    return x * torch.rsqrt((x * x).mean(dim=1, keepdim=True) + EPS)


def _pn_bwd64(g, x, create_graph=False):
    """The first-order gradient of the float64 forward, by autograd: (gx, the leaf x it hangs on)."""
    xl = x.detach().clone().requires_grad_(True)
    return torch.autograd.grad(_pixel_norm64(xl), xl, g, create_graph=create_graph)[0], xl


def _stddev64(x):
    """ops.py:336-348, groups of 4: sample i * M + j is member i of column j; the statistic of a column, on every pixel of its members."""
    b, ch, h, w = x.shape
    y = x.reshape(4, b // 4, ch, h, w)
    y = y - y.mean(dim=0, keepdim=True)
    s = torch.sqrt((y * y).mean(dim=0) + EPS).mean(dim=(1, 2, 3))        # [M]
    return s.reshape(1, -1, 1, 1, 1).expand(4, b // 4, 1, h, w).reshape(b, 1, h, w)


def _stddev_ref(c, d):
    sub = c.args.get("sub", 1)
    outs = []
    for x, gy, ggx, ad in zip(*(d[k].double().chunk(sub) for k in ("x", "gy", "ggx", "addend"))):
        xl, gyl = x.clone().requires_grad_(True), gy.clone().requires_grad_(True)
        y = _stddev64(xl)
        if c.op == OP_STDDEV_FWD:
            outs.append({"y": y.detach()})
            continue
        gx = torch.autograd.grad(y, xl, gyl, create_graph=True)[0]
        if c.op == OP_STDDEV_BWD:
            outs.append({"gx": (gx + ad if c.args["addend"] else gx).detach()})
            continue
        ggy, gx2 = torch.autograd.grad((ggx * gx).sum(), (gyl, xl))
        outs.append({"ggy": ggy, "gx2": gx2})
    return {k: torch.cat([o[k] for o in outs]) for k in outs[0]}


def reference(c, d):
    """name -> float64 result, from the definition of the operation."""
    a = c.args
    acc0 = d["acc0"].double() if a.get("accumulate") else 0.0
    if c.op == OP_BIAS_ACT:
        v = d["x"].double() + (d["bias"].double() if a["bias"] else 0.0)
        return {"y": torch.tanh(v) if a["act"] == TANH else (_lrelu(v) if a["act"] == LRELU else v)}
    if c.op == OP_ACT_BWD:
        return {"gx": d["g"].double() * _dact(d["y"].double(), a["act"])}
    if c.op == OP_TANH_BWD_BWD:   # d/dy [g (1 - y^2)] gg
        y = d["y"].double().requires_grad_(True)
        return {"out": torch.autograd.grad(d["g"].double() * (1.0 - y * y), y, d["gg"].double())[0]}
    if c.op in (OP_AXPBY, OP_AXPBY_DEV):
        return {"out": d["ca"].double() * d["a"].double() + d["cb"].double() * d["b"].double()}
    if c.op == OP_ROW_SCALE:
        return {"out": torch.tensor(a["alpha"], dtype=torch.float32).double() * d["s"].double()[:, None] * d["x"].double()}
    if c.op == OP_UPSCALE:   # the index map: output (oy, ox) reads input (oy // fy, ox // fx)
        n, ch, h, w = c.shape
        oy, ox = torch.arange(h * a["fy"]) // a["fy"], torch.arange(w * a["fx"]) // a["fx"]
        return {"y": d["x"].double()[:, :, oy][:, :, :, ox] * a["scale"]}
    if c.op == OP_BLOCKSUM:
        n, ch, h, w = c.shape
        return {"y": d["x"].double().reshape(n, ch, h, a["fy"], w, a["fx"]).sum(dim=(3, 5)) * torch.tensor(a["scale"], dtype=torch.float32).double()}
    if c.op == OP_CHANNEL_SUM:
        return {"gb": d["g"].double().sum(dim=0) + acc0}
    if c.op == OP_ACT_BWD_BIAS:
        gx = d["g"].double() * _dact(d["y"].double(), a["act"])
        return {"gx": gx, "gb": gx.sum(dim=0) + acc0}
    if c.op == OP_PN_FWD:
        return {"y": _pixel_norm64(d["x"].double())}
    if c.op in (OP_PN_BWD, OP_PN_BWD_BIAS):
        x = d["x"].double()
        gx, _ = _pn_bwd64(d["g"].double() * _dact(x, a["pre"]), x)
        gx = (gx + (d["addend"].double() if a["addend"] else 0.0)) * _dact(x, a["post"])
        return {"gx": gx, "gb": gx.sum(dim=0) + acc0} if c.op == OP_PN_BWD_BIAS else {"gx": gx}
    if c.op == OP_PN_BWD_BWD:   # d <gg', bwd(g, x)> / dx, and bwd(gg', x)
        x = d["x"].double()
        ggp = d["gg"].double() * _dact(x, a["pre"])
        gx, xl = _pn_bwd64(d["g"].double(), x, create_graph=True)
        out = {"out": torch.autograd.grad((ggp * gx).sum(), xl)[0]}
        if a["out2"]:
            out["out2"] = _pn_bwd64(ggp, x)[0]
        return out
    if c.op == OP_SUMSQ_ROWS:
        return {"out": (d["x"].double() ** 2).sum(dim=1)}
    return _stddev_ref(c, d)


def run(K, c, d):
    """The case through its public entry point (gansynth_amd.kernels.HipKernels): name -> result tensor."""
    a = c.args

    def dev(t):
        t = t.to("cuda")
        return t.contiguous(memory_format=torch.channels_last) if t.dim() == 4 else t
    acc = dev(d["acc0"].clone()) if a.get("accumulate") else None
    if c.op == OP_BIAS_ACT:
        return {"y": K.bias_act_fwd(dev(d["x"]), dev(d["bias"]) if a["bias"] else None, a["act"])}
    if c.op == OP_ACT_BWD:
        return {"gx": K.act_bwd(dev(d["g"]), dev(d["y"]), a["act"])}
    if c.op == OP_TANH_BWD_BWD:
        return {"out": K.tanh_bwd_bwd(dev(d["gg"]), dev(d["g"]), dev(d["y"]))}
    if c.op == OP_AXPBY:
        return {"out": K.axpby(dev(d["a"]), dev(d["b"]), float(d["ca"]), float(d["cb"]))}
    if c.op == OP_AXPBY_DEV:
        from gansynth_amd import functional as F
        lerp = F.DeviceLerp("cuda")
        lerp.set(0.3)
        assert torch.equal(lerp.host[:2], torch.stack([d["ca"], d["cb"]]))
        wa, wb = lerp.weights()
        out = K.axpby(dev(d["a"]), dev(d["b"]), wa, wb)
        torch.cuda.synchronize()
        return {"out": out}
    if c.op == OP_ROW_SCALE:
        return {"out": K.row_scale(dev(d["x"]), dev(d["s"]), a["alpha"])}
    if c.op == OP_UPSCALE:
        return {"y": K.upscale2d(dev(d["x"]), a["fy"], a["fx"], a["scale"])}
    if c.op == OP_BLOCKSUM:
        return {"y": K.blocksum2d(dev(d["x"]), a["fy"], a["fx"], a["scale"])}
    if c.op == OP_CHANNEL_SUM:
        return {"gb": K.channel_sum(dev(d["g"]), out=acc)}
    if c.op == OP_ACT_BWD_BIAS:
        gx, gb = K.act_bwd_bias(dev(d["g"]), dev(d["y"]), a["act"], out=acc)
        return {"gx": gx, "gb": gb}
    if c.op == OP_PN_FWD:
        return {"y": K.pixel_norm_fwd(dev(d["x"]), EPS)}
    if c.op == OP_PN_BWD:
        return {"gx": K.pixel_norm_bwd(dev(d["g"]), dev(d["x"]), EPS, act=a["post"], pre_act=a["pre"], addend=dev(d["addend"]) if a["addend"] else None)}
    if c.op == OP_PN_BWD_BIAS:   # (the entry point always adds: "accumulate off" starts from zeros)
        gb = acc if acc is not None else torch.zeros(c.shape[1], device="cuda")
        gx = K.pixel_norm_bwd(dev(d["g"]), dev(d["x"]), EPS, act=a["post"], pre_act=a["pre"], addend=dev(d["addend"]) if a["addend"] else None, bias_out=gb)
        return {"gx": gx, "gb": gb}
    if c.op == OP_PN_BWD_BWD:
        res = K.pixel_norm_bwd_bwd(dev(d["gg"]), dev(d["g"]), dev(d["x"]), EPS, pre_act=a["pre"], with_g=bool(a["out2"]))
        return {"out": res[0], "out2": res[1]} if a["out2"] else {"out": res}
    if c.op == OP_SUMSQ_ROWS:
        return {"out": K.sumsq_rows(dev(d["x"]))}
    sub = a.get("sub", 1)
    if c.op == OP_STDDEV_FWD:
        return {"y": K.batch_stddev_fwd(dev(d["x"]), EPS, sub=sub)}
    if c.op == OP_STDDEV_BWD:
        return {"gx": K.batch_stddev_bwd(dev(d["gy"]), dev(d["x"]), EPS, addend=dev(d["addend"]) if a["addend"] else None, sub=sub)}
    ggy, gx2 = K.batch_stddev_bwd_bwd(dev(d["ggx"]), dev(d["gy"]), dev(d["x"]), EPS, sub=sub)
    return {"ggy": ggy, "gx2": gx2}


def ratio(got, ref):
    return igemm_cover.ratio(got, ref)


def within(c, name, got, ref):
    """(ratio, ok): the suite's measure under the family's ceiling.  A bf16 result: the element-wise bound of one rounding instead (which keeps the
    ratio under 2^-8 + ceiling); upscale at scale 1: the bits of the reference rounded to the dtype."""
    ceil = ceiling(c.op, name)
    r = ratio(got, ref)
    if c.op == OP_UPSCALE and c.args["scale"] == 1.0:
        return r, torch.equal(got.detach().cpu(), ref.to(got.dtype))
    if got.dtype == torch.bfloat16:
        g, f = got.detach().double().cpu(), ref.detach().double().cpu()
        return r, bool(((g - f).abs() <= 2.0 ** -8 * f.abs() + ceil * float(f.abs().max())).all())
    return r, r <= ceil
