"""The cases of the pitch classifier's kernels (csrc/classifier.hip, csrc/classifier_bwd.hip) -- shared by tests/test_classifier_cover_cpu.py and
tests/test_classifier_cover_gpu.py (a plain helper module: no fixtures, no collection hooks).

KERNELS is the list of the 40 compiled instantiations as the launchers spell them.  A case is an operation, a dtype, a shape, what is asked of it
(args), the instantiation `key` it is there for and `want`: the geometry facts that make it the case it claims to be (S=6, tail_slice=14, trips=2,
splits=9, last_split_rows=46 ...).  These kernels have no route function: what a launch does is decided by host arithmetic inside the entry
points, restated here (gn_geometry, conv1x1_wgrad_split, stem_wgrad_blocks, momentum_blocks, the block caps of the grid-stride launches, the
stem's pool-tile grid).  The CPU test holds the restatement against the byte counts the library's *_workspace_bytes functions answer, and every
case's `want` against `facts`.

`reference` is float64 on the operands as stored (activations rounded to bf16 first for bf16; weights, statistics, gamma, beta fp32), written from
the definition of each operation; backward references are torch.autograd of the float64 forward (tests/resnet_ref.py where it has the block).  The
two large grid-stride group-norm cases use the closed form `gn_relu_bwd_closed` (held against autograd by the CPU test on every small case).  The
statistics a group-norm apply / backward case hands the kernel are the float64 ones rounded to fp32, so every kernel is measured on its own.

fold_partials_kernel is reached with S in {1, 3, 4, 9, 1024} (conv1x1 weight gradients of 1, 3 and 9 splits, stem weight gradients of 4 and 1024
blocks).  Its `i < N` guard cannot be reached from any entry point: N is ci * co or 99 * 64, always a multiple of 64.

Bounds.  GEMM-like kernels (1x1 forward / data / weight, stem forward / weight gradient), element by element:
    |got - ref| <= (K + 2) 2^-24 sum_k |a_k| |b_k|        K: the reduction length; the sum: the same reference on absolute values
(K fused multiply-adds and at most two more roundings: the bias or the accumulate add, the fold).  Everything else: a ceiling of max |ref| per
family, the suite's own (1e-3; 1e-4 the group mean; 1e-5 the standardised weight; 1e-6 the max-pool gradient and l2) tightened to 16 times the worst
error measured on the MI355X against the float64 reference, rounded up to a power of ten and never above the suite's own.  A bf16 result is
computed in fp32 and rounded once on the store: |got - ref| <= 2^-8 |ref| + the fp32 bound, element by element.  fp32 results of bf16 operands
(statistics, dgamma, dbeta, weight gradients, features) take the fp32 bound.  ReLU decisions: elements whose float64 pre-activation has
|pre| < 1e-5 max |pre| are left out of the dx comparison only (their share is at most 0.1 %, asserted by the CPU test, 0 on the small cases);
dgamma / dbeta are compared whole, at their ceilings and nothing more.

The backward of a two-row standardisation (fan_in = 2) is the one place where the cover cannot hold the kernel at an ordinary input: two rows
standardise to +-1 whatever they hold, the exact gradient is zero but for eps (about 1e-8 at a spread of 0.05), and the kernel, which reads the
standardised weight back in fp32, answers with rounding noise of that size -- about 1e-8 absolute, about 100 % of a reference that is itself
nothing.  The case gives that weight a spread of the size of sqrt(eps), where the gradient is of order 1 and the comparison means something.

Worst errors over max |ref| measured on the MI355X over seeds 0 .. 11 of every small case and seed 0 of the large ones (fp32 results only: a
bf16 result adds its own rounding, which the bound carries; test_classifier_cover_gpu.py runs those seeds and prints the column:
CLASSIFIER-COVER-WORST), the suite's ceiling and the ceiling held here (CEILINGS below; the CPU test holds the two copies together):
    family            measured    suite   here
    gn_mean           3.6e-07     0.0001  1e-05
    gn_rstd           2.1e-07     0.001   1e-05
    gn_apply          1.2e-07     0.001   1e-05
    gn_head           1.7e-07     0.001   1e-05
    gn_bwd_dx         1.4e-06     0.001   0.0001
    gn_bwd_dgamma     5.7e-07     0.001   1e-05
    gn_bwd_dbeta      3.0e-07     0.001   1e-05
    max_pool_bwd      9.8e-08     1e-06   1e-06
    ws_out            5.1e-08     1e-05   1e-06
    ws_rstd           4.1e-08     1e-05   1e-06
    ws_bwd            1.0e-07     0.001   1e-05
    xent_loss         2.0e-07     0.001   1e-05
    xent_dlogits      8.2e-07     0.001   0.0001
    momentum_p        4.9e-08     0.001   1e-06
    momentum_accum    8.0e-08     0.001   1e-05
    momentum_l2       5.1e-08     1e-06   1e-06
"""
import ctypes
import zlib
from collections import namedtuple

import numpy as np
import torch

from tests import resnet_ref as RR

F32, BF16 = 0, 1
DTYPES = (F32, BF16)
DTYPE_NAMES = ("f32", "bf16")
TORCH_DTYPE = {F32: torch.float32, BF16: torch.bfloat16}
ERR_ARG, ERR_WORKSPACE = -1, -4
EPS = RR.EPS
GN_GRID_CAP, POOL_GRID_CAP, POOL_BWD_GRID_CAP = 16384, 8192, 16384     # gs_group_norm_apply / gnb_dx, gs_max_pool2d, gs_max_pool2d_bwd
STEM_PR, STEM_PC = 2, 16                                                # pool outputs of a stem tile
STEMB_TW, STEMB_MAXB, MOM_MAXB = 32, 1024, 1024
WS_CH, WS_RL = 16, 16
UNDECIDED = 1e-5

# family -> (worst measured on the MI355X, the suite's ceiling, the ceiling held here = min(suite, 16 x measured rounded up to a power of ten)):
# the table of the docstring
CEILINGS = {
    "gn_mean":        (3.6e-07, 0.0001, 1e-05),
    "gn_rstd":        (2.1e-07, 0.001, 1e-05),
    "gn_apply":       (1.2e-07, 0.001, 1e-05),
    "gn_head":        (1.7e-07, 0.001, 1e-05),
    "gn_bwd_dx":      (1.4e-06, 0.001, 0.0001),
    "gn_bwd_dgamma":  (5.7e-07, 0.001, 1e-05),
    "gn_bwd_dbeta":   (3.0e-07, 0.001, 1e-05),
    "max_pool_bwd":   (9.8e-08, 1e-06, 1e-06),
    "ws_out":         (5.1e-08, 1e-05, 1e-06),
    "ws_rstd":        (4.1e-08, 1e-05, 1e-06),
    "ws_bwd":         (1.0e-07, 0.001, 1e-05),
    "xent_loss":      (2.0e-07, 0.001, 1e-05),
    "xent_dlogits":   (8.2e-07, 0.001, 0.0001),
    "momentum_p":     (4.9e-08, 0.001, 1e-06),
    "momentum_accum": (8.0e-08, 0.001, 1e-05),
    "momentum_l2":    (5.1e-08, 1e-06, 1e-06),
}
assert all(here <= suite for _, suite, here in CEILINGS.values())
SEEDS = tuple(range(12))   # of the measurement: every small case at each, the large ones at SEEDS[0]

Key = namedtuple("Key", "kernel dtype flag")   # one compiled instantiation; dtype None: not a template; flag: ADD / HEAD
Case = namedtuple("Case", "op dtype shape args key want")


def _key(kernel, dtype=None, flag=None):
    return Key(kernel, dtype, flag)


KERNELS = (
    # classifier.hip: 16
    [_key("weight_std"), _key("gn_finalize")]
    + [_key(k, d) for d in DTYPES for k in ("stem_pool", "max_pool", "conv1x1", "gn_apply", "gn_relu_mean")]
    + [_key("gn_partial", d, add) for d in DTYPES for add in (False, True)]
    # classifier_bwd.hip: 24
    + [_key(k) for k in ("fold_partials", "gnb_finalize", "gnb_param", "weight_std_batch", "weight_std_bwd_batch", "softmax_xent", "momentum", "momentum_l2")]
    + [_key(k, d, head) for d in DTYPES for k in ("gnb_partial", "gnb_dx") for head in (False, True)]
    + [_key(k, d) for d in DTYPES for k in ("max_pool_bwd", "stem_wgrad", "conv1x1_bwd_data", "conv1x1_bwd_weight")]
)
assert len(KERNELS) == len(set(KERNELS)) == 40


def key_id(k):
    return "-".join([k.kernel] + ([DTYPE_NAMES[k.dtype]] if k.dtype is not None else []) + ([str(k.flag).lower()] if k.flag is not None else []))


def case_id(c):
    args = "+".join(f"{k}={v}" for k, v in sorted(c.args.items()))
    return f"{c.op}-{DTYPE_NAMES[c.dtype]} {'x'.join(str(v) for v in c.shape)} {args}".rstrip()


def case_keys(c):
    """The instantiations a case launches."""
    d, a = c.dtype, c.args
    if c.op == "gn_stats":
        return {_key("gn_partial", d, bool(a["addend"])), _key("gn_finalize")}
    if c.op in ("gn_bwd", "gn_head_bwd"):
        head = c.op == "gn_head_bwd"
        return {_key("gnb_partial", d, head), _key("gnb_finalize"), _key("gnb_param"), _key("gnb_dx", d, head)}
    if c.op in ("conv1x1_bwd_weight", "stem_wgrad"):
        return {_key(c.op, d), _key("fold_partials")}
    if c.op == "weight_std":
        return {_key("weight_std"), _key("weight_std_batch"), _key("weight_std_bwd_batch")}
    if c.op == "momentum":
        return {_key("momentum")} | ({_key("momentum_l2")} if a["want_l2"] else set())
    return {_key({"gn_head": "gn_relu_mean", "conv1x1_fwd": "conv1x1"}.get(c.op, c.op), None if c.op == "softmax_xent" else d)}


# ------------------------------------------------------------------------------------------------- the host arithmetic, restated
def _cdiv(a, b):
    return -(-a // b)


def gn_geometry(n, hw, c):
    """classifier_shared.h: gn_geometry -> (S, pps): S slices of pps pixels per image; R = 1024 / c pixel rows per block."""
    R = 1024 // c
    s = max(1, min(2048 // max(n, 1), hw // (4 * R)))
    pps = _cdiv(hw, s)
    return _cdiv(hw, pps), pps


def gn_workspace_bytes(n, hw, c, groups):
    return n * gn_geometry(n, hw, c)[0] * groups * 12


def gn_bwd_workspace_bytes(n, hw, c, groups):
    return (n * gn_geometry(n, hw, c)[0] * c + n * c + n * groups) * 8


def grid_stride(total, cap):
    """(blocks, trips) of a 256-thread grid-stride launch over `total` items."""
    blocks = min(_cdiv(total, 256), cap)
    return blocks, _cdiv(total, blocks * 256)


def conv1x1_wgrad_split(M, ci, co):
    """classifier_bwd.hip: conv1x1_wgrad_split -> (splits, rows)."""
    ks = max(1, 512 // ((ci // 64) * (co // 64)))
    chunks = _cdiv(M, 32)
    ks = min(ks, chunks)
    rows = _cdiv(chunks, ks) * 32
    return _cdiv(M, rows), rows


def conv1x1_wgrad_workspace_bytes(n, h, w, ci, co, stride):
    return conv1x1_wgrad_split(n * (h // stride) * (w // stride), ci, co)[0] * ci * co * 4


def stem_wgrad_blocks(n, h, w):
    """-> (tiles, blocks, trips): tiles of one stem row x 32 columns, walked by at most 1024 blocks."""
    tiles = n * (h // 2) * _cdiv(w // 2, STEMB_TW)
    blocks = min(tiles, STEMB_MAXB)
    return tiles, blocks, _cdiv(tiles, blocks)


def stem_wgrad_workspace_bytes(n, h, w):
    return stem_wgrad_blocks(n, h, w)[1] * 99 * 64 * 4


def momentum_blocks(n):
    """-> (blocks, trips) over the n / 4 vectors."""
    blocks = max(1, min(_cdiv(n // 4, 1024), MOM_MAXB))
    return blocks, _cdiv(n // 4, blocks * 256)


def momentum_workspace_bytes(n):
    return momentum_blocks(n)[0] * 8


def stem_pool_grid(n, h, w):
    return _cdiv(w // 4, STEM_PC), _cdiv(h // 4, STEM_PR), n


def facts(c):
    """The geometry facts of a case under the restated arithmetic: what `want` may name."""
    a, f = c.args, {}
    if c.op.startswith("gn_"):
        n, ch, h, w, G = c.shape
        hw, R = h * w, 1024 // ch
        S, pps = gn_geometry(n, hw, ch)
        tail = hw - (S - 1) * pps
        blocks, trips = grid_stride(n * hw * ch // 4, GN_GRID_CAP)
        f.update(R=R, S=S, pps=pps, tail_slice=0 if tail == pps else tail, S_mod_4=S % 4, hw_lt_R=int(hw < R), cg=ch // G, c_lt_64=int(ch < 64), n=n,
                 blocks=blocks, trips=trips, ragged_trip=int(trips > 1 and (n * hw * ch // 4) % (blocks * 256) != 0), idle_waves=max(0, 4 - hw),
                 accumulate=int(a.get("accumulate", 0)), addend=int(a.get("addend", 0)))
    elif c.op.startswith("conv1x1"):
        ci, co, stride, n, h, w = c.shape
        M = n * (h // stride) * (w // stride)
        splits, rows = conv1x1_wgrad_split(M, ci, co) if ci % 64 == 0 else (0, 0)   # (the forward alone admits ci % 64 == 32)
        last = M - (splits - 1) * rows
        f.update(M=M, m_tiles=_cdiv(M, 64), last_tile_rows=M - 64 * (_cdiv(M, 64) - 1), M_mod_64=M % 64, splits=splits, rows=rows, last_split_rows=last,
                 zero_rows=int(splits > 0 and last % 32 != 0), ci_mod_64=ci % 64, stride=stride, out=int(a.get("out", 0)))
    elif c.op == "stem_pool":
        n, h, w = c.shape
        gx, gy, _ = stem_pool_grid(n, h, w)
        f.update(Hp=h // 4, Wp=w // 4, grid_x=gx, grid_y=gy, partial_x=(w // 4) % STEM_PC, partial_y=(h // 4) % STEM_PR, want_pool=int(a["want_pool"]),
                 bias=int(a["bias"]))
    elif c.op == "stem_wgrad":
        n, h, w = c.shape
        tiles, blocks, trips = stem_wgrad_blocks(n, h, w)
        f.update(tiles=tiles, blocks=blocks, trips=trips, second_tile_blocks=tiles - blocks if trips == 2 else 0, Ws=w // 2, last_col_tile=(w // 2) % STEMB_TW,
                 col_tiles=_cdiv(w // 2, STEMB_TW), out=int(a["out"]))
    elif c.op in ("max_pool", "max_pool_bwd"):
        n, ch, h, w = c.shape
        total = n * (h // 2) * (w // 2) * ch if c.op == "max_pool" else n * h * w * ch
        blocks, trips = grid_stride(total, POOL_GRID_CAP if c.op == "max_pool" else POOL_BWD_GRID_CAP)
        f.update(blocks=blocks, trips=trips, odd=int(h % 2 == 1 and w % 2 == 1), ties=int(a.get("ties", 0)))
    elif c.op == "weight_std":
        f.update(ragged_channels=int(any(s[-1] % WS_CH for s in c.shape)), short_fan=int(any(_fan(s) < WS_RL for s in c.shape)),
                 fan_1=int(any(_fan(s) == 1 for s in c.shape)), weights=len(c.shape), idle_blocks=int(len({_cdiv(s[-1], WS_CH) for s in c.shape}) > 1))
    elif c.op == "softmax_xent":
        f.update(trips=_cdiv(c.shape[0], 256), ragged_trip=int(c.shape[0] > 256 and c.shape[0] % 256 != 0), soft=int(a["soft"]), want_grad=int(a["want_grad"]),
                 ties=int(a["ties"]))
    elif c.op == "momentum":
        blocks, trips = momentum_blocks(c.shape[0])
        lo, hi = a["lo"], a["hi"]
        f.update(blocks=blocks, trips=trips, ragged_trip=int((c.shape[0] // 4) % (blocks * 256) != 0), lo_mod_4=lo % 4, hi_mod_4=hi % 4, empty=int(lo == hi),
                 nesterov=int(a["nesterov"]), zero_grad=int(a["zero_grad"]), want_l2=int(a["want_l2"]))
    return f


def is_large(c):
    """The cases that run at one seed only: the grid-stride loops at their caps."""
    return bool(c.args.get("large")) or c.op == "momentum" or (c.op in ("max_pool", "max_pool_bwd") and int(np.prod(c.shape)) > 1 << 20)


def _fan(shape):
    return int(np.prod(shape[:-1]))


# ---------------------------------------------------------------------------------------------------------------------------------- the cases
GN_SHAPES = {   # (n, c, h, w, groups) -> the facts it is there for
    (2, 4, 3, 5, 2): dict(R=256, hw_lt_R=1, S=1, c_lt_64=1),
    (2, 32, 5, 7, 32): dict(cg=1, c_lt_64=1, S=1),
    (2, 256, 9, 11, 4): dict(cg=64, S=6, pps=17, tail_slice=14, S_mod_4=2),
    (1, 1024, 3, 6, 16): dict(R=1, S=4, pps=5, tail_slice=3, cg=64),
    (3, 64, 8, 32, 32): dict(n=3, S=4, pps=64, tail_slice=0, cg=2),
}
HEAD_SHAPES = {(2, 256, 9, 11, 4): GN_SHAPES[(2, 256, 9, 11, 4)], (1, 1024, 3, 6, 16): GN_SHAPES[(1, 1024, 3, 6, 16)], (2, 64, 1, 2, 32): dict(idle_waves=2, S=1)}
GN_LARGE = (2, 4, 3, 699057, 2)   # 2 x 2097171 pixels of 4 channels: 38 vectors past 16384 x 256
CONV1X1_SHAPES = {   # (ci, co, stride, n, h, w)
    (64, 64, 1, 2, 3, 5): dict(M=30, m_tiles=1, last_tile_rows=30, splits=1, last_split_rows=30, zero_rows=1),
    (64, 64, 1, 2, 5, 7): dict(M=70, m_tiles=2, last_tile_rows=6, splits=3, last_split_rows=6),
    (256, 512, 2, 2, 18, 62): dict(M=558, splits=9, rows=64, last_split_rows=46, stride=2),
    (128, 64, 2, 1, 2, 2): dict(M=1, splits=1, stride=2),
}
CONV1X1_FWD_ONLY = {(32, 64, 1, 2, 5, 7): dict(M=70, ci_mod_64=32), (96, 64, 1, 2, 5, 7): dict(M=70, ci_mod_64=32)}
STEM_FWD_SHAPES = {(2, 4, 4): dict(Hp=1, Wp=1, partial_y=1, partial_x=1), (1, 12, 72): dict(Hp=3, Wp=18, grid_x=2, grid_y=2, partial_y=1, partial_x=2)}
STEM_WGRAD_SHAPES = {(2, 4, 4): dict(Ws=2, tiles=4, blocks=4, trips=1), (1, 12, 72): dict(Ws=36, col_tiles=2, last_col_tile=4),
                     (5, 512, 4): dict(tiles=1280, blocks=1024, trips=2, second_tile_blocks=256)}
WS_SHAPES = ((1, 1, 1, 7), (1, 1, 2, 61), (3, 3, 5, 16), (1, 1, 40, 33), (7, 7, 2, 64))
MOM_N = 4 * (1024 * 1024) + 4 * 37


def _cases():
    out = []

    def add(op, d, shape, key, want=None, **args):
        out.append(Case(op, d, tuple(shape), args, _key(*key), dict(want or {})))
    for d in DTYPES:
        # ---- group norm: statistics (with and without the residual add), apply, ReLU backward (addend; accumulate into non-zero buffers)
        for shape, want in GN_SHAPES.items():
            for addend in (0, 1):
                add("gn_stats", d, shape, ("gn_partial", d, bool(addend)), dict(want, addend=addend), addend=addend)
                add("gn_bwd", d, shape, ("gnb_partial", d, False), dict(want, addend=addend, accumulate=0), addend=addend, accumulate=0)
            add("gn_bwd", d, shape, ("gnb_dx", d, False), dict(want, accumulate=1), addend=0, accumulate=1)
            for relu in (1, 0):
                add("gn_apply", d, shape, ("gn_apply", d), want, relu=relu)
        for shape, want in HEAD_SHAPES.items():
            add("gn_head", d, shape, ("gn_relu_mean", d), want)
            for acc in (0, 1):
                add("gn_head_bwd", d, shape, ("gnb_partial", d, True), dict(want, accumulate=acc), accumulate=acc)
        # ---- 1x1 projection: forward, data gradient (written, added into), weight gradient (written, added into)
        for shape, want in CONV1X1_SHAPES.items():
            add("conv1x1_fwd", d, shape, ("conv1x1", d), want)
            for o in (0, 1):
                add("conv1x1_bwd_data", d, shape, ("conv1x1_bwd_data", d), dict(want, out=o), out=o)
                add("conv1x1_bwd_weight", d, shape, ("conv1x1_bwd_weight", d), dict(want, out=o), out=o)
        for shape, want in CONV1X1_FWD_ONLY.items():
            add("conv1x1_fwd", d, shape, ("conv1x1", d), want)
        # ---- stem: forward with the pool (options), weight gradient
        for shape, want in STEM_FWD_SHAPES.items():
            for want_pool, bias in ((1, 1), (0, 1), (1, 0)):
                add("stem_pool", d, shape, ("stem_pool", d), dict(want, want_pool=want_pool, bias=bias), want_pool=want_pool, bias=bias)
        for shape, want in STEM_WGRAD_SHAPES.items():
            for o in (0, 1):
                add("stem_wgrad", d, shape, ("stem_wgrad", d), dict(want, out=o), out=o)
        # ---- max pool
        add("max_pool", d, (2, 8, 2, 2), ("max_pool", d), dict(trips=1))
        add("max_pool", d, (2, 64, 8, 32), ("max_pool", d), dict(trips=1))
        for shape in ((1, 64, 1, 1), (2, 8, 2, 3), (2, 64, 7, 31)):
            add("max_pool_bwd", d, shape, ("max_pool_bwd", d), dict(trips=1))
        add("max_pool_bwd", d, (2, 64, 7, 31), ("max_pool_bwd", d), dict(trips=1, ties=1, odd=1), ties=1)
    # ---- the grid-stride loops at their caps, once each (fp32)
    add("gn_apply", F32, GN_LARGE, ("gn_apply", F32), dict(blocks=16384, trips=2, ragged_trip=1, R=256, S=1024), relu=1, large=1)
    add("gn_bwd", F32, GN_LARGE, ("gnb_dx", F32, False), dict(blocks=16384, trips=2, ragged_trip=1, S=1024, tail_slice=1044), addend=1, accumulate=0, large=1)
    add("max_pool", F32, (1, 64, 258, 510), ("max_pool", F32), dict(blocks=8192, trips=2))
    add("max_pool_bwd", F32, (1, 64, 257, 257), ("max_pool_bwd", F32), dict(blocks=16384, trips=2, odd=1))
    # ---- weight standardisation: the per-weight launch, the batched launch and its backward over one table of mixed widths
    add("weight_std", F32, WS_SHAPES, ("weight_std_batch",), dict(ragged_channels=1, short_fan=1, fan_1=1, idle_blocks=1, weights=5))
    # ---- softmax cross-entropy
    for n in (1, 256, 257, 600):
        for soft in (0, 1):
            add("softmax_xent", F32, (n, 61), ("softmax_xent",), dict(trips=_cdiv(n, 256), soft=soft, ties=1), soft=soft, want_grad=1, ties=1)
    add("softmax_xent", F32, (600, 61), ("softmax_xent",), dict(trips=3, ragged_trip=1, want_grad=0), soft=1, want_grad=0, ties=1)
    # ---- momentum: capped blocks and a ragged fifth trip; a range over everything, one that starts and ends inside a 4-vector, an empty one
    mom = dict(blocks=1024, trips=5, ragged_trip=1)
    add("momentum", F32, (MOM_N,), ("momentum",), dict(mom, lo_mod_4=0), lo=0, hi=MOM_N, nesterov=1, zero_grad=1, want_l2=1)
    add("momentum", F32, (MOM_N,), ("momentum",), dict(mom, lo_mod_4=1, hi_mod_4=3), lo=5, hi=4 * 1024 * 1024 + 3, nesterov=0, zero_grad=1, want_l2=1)
    add("momentum", F32, (MOM_N,), ("momentum",), dict(mom, lo_mod_4=1, zero_grad=0), lo=5, hi=4 * 1024 * 1024 + 3, nesterov=1, zero_grad=0, want_l2=1)
    add("momentum", F32, (MOM_N,), ("momentum_l2",), dict(mom, empty=1), lo=8, hi=8, nesterov=1, zero_grad=1, want_l2=1)
    add("momentum", F32, (MOM_N,), ("momentum",), dict(mom, empty=1, want_l2=0), lo=8, hi=8, nesterov=0, zero_grad=0, want_l2=0)
    add("momentum", F32, (MOM_N,), ("momentum",), dict(mom, want_l2=0), lo=0, hi=MOM_N, nesterov=1, zero_grad=1, want_l2=0)
    return out


CASES = _cases()

# What the suite did not notice before this cover: (fact, ops it must be seen on, a predicate on (case, facts)).  Every entry
# needs a case in each dtype that has the kernel (fp32 alone where `f32_only`).
REQUIRED = [
    ("gn: a short last slice", ("gn_stats", "gn_bwd", "gn_head_bwd"), lambda c, f: f["tail_slice"] > 0, False),
    ("gn: S not a multiple of 4", ("gn_stats", "gn_bwd", "gn_head_bwd"), lambda c, f: f["S_mod_4"] != 0 and f["S"] > 1, False),
    ("gn: hw < R", ("gn_stats", "gn_bwd"), lambda c, f: f["hw_lt_R"] == 1, False),
    ("gn: c = 4 (R = 256)", ("gn_stats", "gn_bwd", "gn_apply"), lambda c, f: f["R"] == 256, False),
    ("gn: c = 1024 (R = 1)", ("gn_stats", "gn_bwd", "gn_apply", "gn_head", "gn_head_bwd"), lambda c, f: f["R"] == 1, False),
    ("gn: c < 64", ("gn_bwd",), lambda c, f: f["c_lt_64"] == 1, False),
    ("gn: 64 channels per group", ("gn_stats", "gn_bwd", "gn_head_bwd"), lambda c, f: f["cg"] == 64, False),
    ("gn: 1 channel per group", ("gn_stats", "gn_bwd"), lambda c, f: f["cg"] == 1, False),
    ("gn: groups != 32", ("gn_stats", "gn_bwd", "gn_apply"), lambda c, f: c.shape[4] != 32, False),
    ("gn: odd batch", ("gn_stats", "gn_bwd"), lambda c, f: f["n"] % 2 == 1 and f["n"] > 1, False),
    ("gn: statistics with addend", ("gn_stats",), lambda c, f: f["addend"] == 1, False),
    ("gn: backward with addend", ("gn_bwd",), lambda c, f: f["addend"] == 1, False),
    ("gn: accumulate = 1", ("gn_bwd", "gn_head_bwd"), lambda c, f: f["accumulate"] == 1, False),
    ("gn: head with idle waves", ("gn_head", "gn_head_bwd"), lambda c, f: f["idle_waves"] > 0, False),
    ("gn_apply: a second grid-stride trip", ("gn_apply",), lambda c, f: f["trips"] == 2 and f["ragged_trip"] == 1, True),
    ("gnb_dx: a second grid-stride trip", ("gn_bwd",), lambda c, f: f["trips"] == 2 and f["ragged_trip"] == 1, True),
    ("conv1x1: M not a multiple of 64", ("conv1x1_fwd", "conv1x1_bwd_data", "conv1x1_bwd_weight"), lambda c, f: f["M_mod_64"] != 0, False),
    ("conv1x1: a ragged second tile", ("conv1x1_fwd", "conv1x1_bwd_data"), lambda c, f: f["m_tiles"] >= 2 and f["last_tile_rows"] < 64, False),
    ("conv1x1: M = 1", ("conv1x1_fwd", "conv1x1_bwd_data", "conv1x1_bwd_weight"), lambda c, f: f["M"] == 1, False),
    ("conv1x1: a short last split", ("conv1x1_bwd_weight",), lambda c, f: f["splits"] > 1 and f["last_split_rows"] < f["rows"], False),
    ("conv1x1: zero-filled loader rows", ("conv1x1_bwd_weight",), lambda c, f: f["zero_rows"] == 1, False),
    ("conv1x1: splits = 1 with me < rows", ("conv1x1_bwd_weight",), lambda c, f: f["splits"] == 1 and f["M"] < f["rows"], False),
    ("conv1x1: ci % 64 = 32", ("conv1x1_fwd",), lambda c, f: f["ci_mod_64"] == 32, False),
    ("conv1x1: stride 2 written, not added", ("conv1x1_bwd_data",), lambda c, f: f["stride"] == 2 and f["out"] == 0, False),
    ("conv1x1: added into out=", ("conv1x1_bwd_data", "conv1x1_bwd_weight"), lambda c, f: f["out"] == 1, False),
    ("fold: S = 1", ("conv1x1_bwd_weight",), lambda c, f: f["splits"] == 1, False),
    ("fold: S = 3", ("conv1x1_bwd_weight",), lambda c, f: f["splits"] == 3, False),
    ("fold: S = 9", ("conv1x1_bwd_weight",), lambda c, f: f["splits"] == 9, False),
    ("fold: S = 4", ("stem_wgrad",), lambda c, f: f["blocks"] == 4, False),
    ("fold: S = 1024", ("stem_wgrad",), lambda c, f: f["blocks"] == 1024, False),
    ("stem_wgrad: more tiles than blocks", ("stem_wgrad",), lambda c, f: f["tiles"] > STEMB_MAXB and f["trips"] == 2, False),
    ("stem_wgrad: a ragged last column tile", ("stem_wgrad",), lambda c, f: f["last_col_tile"] != 0 and f["col_tiles"] > 1, False),
    ("stem_wgrad: added into out=", ("stem_wgrad",), lambda c, f: f["out"] == 1, False),
    ("stem_pool: a partial tile in both directions", ("stem_pool",), lambda c, f: f["partial_x"] and f["partial_y"] and f["grid_x"] > 1 and f["grid_y"] > 1, False),
    ("stem_pool: Hp < STEM_PR", ("stem_pool",), lambda c, f: f["Hp"] < STEM_PR, False),
    ("stem_pool: want_pool=False", ("stem_pool",), lambda c, f: f["want_pool"] == 0, False),
    ("stem_pool: bias=None", ("stem_pool",), lambda c, f: f["bias"] == 0, False),
    ("max_pool: a second grid-stride trip", ("max_pool",), lambda c, f: f["trips"] == 2, True),
    ("max_pool_bwd: a second grid-stride trip on an odd size", ("max_pool_bwd",), lambda c, f: f["trips"] == 2 and f["odd"] == 1, True),
    ("max_pool_bwd: ties", ("max_pool_bwd",), lambda c, f: f["ties"] == 1, False),
    ("weight_std: co % WS_CH != 0", ("weight_std",), lambda c, f: f["ragged_channels"] == 1, True),
    ("weight_std: fan_in < WS_RL", ("weight_std",), lambda c, f: f["short_fan"] == 1, True),
    ("weight_std: fan_in = 1", ("weight_std",), lambda c, f: f["fan_1"] == 1, True),
    ("softmax_xent: N > 256", ("softmax_xent",), lambda c, f: f["trips"] > 1 and f["ragged_trip"] == 1, True),
    ("softmax_xent: soft labels", ("softmax_xent",), lambda c, f: f["soft"] == 1, True),
    ("softmax_xent: argmax ties", ("softmax_xent",), lambda c, f: f["ties"] == 1, True),
    ("softmax_xent: want_grad=False", ("softmax_xent",), lambda c, f: f["want_grad"] == 0, True),
    ("momentum: capped blocks, several trips", ("momentum",), lambda c, f: f["blocks"] == MOM_MAXB and f["trips"] > 1 and f["ragged_trip"] == 1, True),
    ("momentum: a range that starts inside a 4-vector", ("momentum",), lambda c, f: f["lo_mod_4"] != 0 and not f["empty"], True),
    ("momentum: an empty range", ("momentum",), lambda c, f: f["empty"] == 1, True),
    ("momentum: zero_grad=False", ("momentum",), lambda c, f: f["zero_grad"] == 0, True),
    ("momentum: want_l2=False", ("momentum",), lambda c, f: f["want_l2"] == 0, True),
    ("momentum: plain", ("momentum",), lambda c, f: f["nesterov"] == 0, True),
    ("momentum: Nesterov", ("momentum",), lambda c, f: f["nesterov"] == 1, True),
]


def missing_facts(cases=None):
    """The entries of REQUIRED (with op and dtype) that no case reaches."""
    cases = CASES if cases is None else cases
    fs = [(c, facts(c)) for c in cases]
    out = []
    for name, ops, pred, f32_only in REQUIRED:
        for op in ops:
            for d in (F32,) if f32_only else DTYPES:
                if not any(c.op == op and c.dtype == d and pred(c, f) for c, f in fs):
                    out.append(f"{name} [{op}-{DTYPE_NAMES[d]}]")
    return out


# --------------------------------------------------------------------------------------------------------------------- operands and reference
def _gen(c, seed):
    return torch.Generator().manual_seed(zlib.crc32(case_id(c).encode()) % (2 ** 31) + seed)


def inputs(c, seed=0):
    """The operands of a case as stored (CPU; activations rounded to the case's dtype, everything else fp32)."""
    g = _gen(c, seed)
    dt = TORCH_DTYPE[c.dtype]
    a = c.args

    def rn(*shape):
        return torch.randn(*shape, generator=g)
    d = {}
    if c.op.startswith("gn_"):
        n, ch, h, w, G = c.shape
        d["x"] = (rn(n, ch, h, w) + rn(1, ch, 1, 1)).to(dt)
        d["gamma"], d["beta"] = 1.0 + 0.3 * rn(ch), 0.2 * rn(ch)
        if c.op == "gn_stats":
            if a["addend"]:
                d["addend"] = (rn(n, ch, h, w) + 1.0).to(dt)
            return d
        if c.op in ("gn_bwd", "gn_head_bwd"):
            if c.op == "gn_bwd":
                d["gy"] = rn(n, ch, h, w).to(dt)
                if a["addend"]:
                    d["addend"] = rn(n, ch, h, w).to(dt)
            else:
                d["gf"] = rn(n, ch)
            if a["accumulate"]:
                d["dgamma0"], d["dbeta0"] = 0.5 * rn(ch) + 0.25, 0.5 * rn(ch) - 0.25
        d["stats"] = RR.group_stats(d["x"].double(), G).float()
    elif c.op.startswith("conv1x1"):
        ci, co, stride, n, h, w = c.shape
        d["w"] = rn(1, 1, ci, co) / ci ** 0.5
        if c.op != "conv1x1_bwd_data":
            d["x"] = rn(n, ci, h, w).to(dt)
        if c.op != "conv1x1_fwd":
            d["gy"] = rn(n, co, h // stride, w // stride).to(dt)
            if a["out"]:
                d["out0"] = rn(n, ci, h, w).to(dt) if c.op == "conv1x1_bwd_data" else 0.5 * rn(1, 1, ci, co)
    elif c.op in ("stem_pool", "stem_wgrad"):
        n, h, w = c.shape
        d["x"] = rn(n, 2, h, w).to(dt)
        if c.op == "stem_pool":
            d["w"] = 0.2 * rn(7, 7, 2, 64)
            if a["bias"]:
                d["bias"] = 0.1 * rn(64)
        else:
            d["gstem"] = rn(n, 64, h // 2, w // 2).to(dt)
            if a["out"]:
                d["gw0"], d["gb0"] = 0.5 * rn(7, 7, 2, 64), 0.5 * rn(64)
    elif c.op in ("max_pool", "max_pool_bwd"):
        d["x"] = (torch.randint(0, 3, c.shape, generator=g).float() if a.get("ties") else rn(*c.shape)).to(dt)
        if c.op == "max_pool_bwd":
            n, ch, h, w = c.shape
            d["gy"] = rn(n, ch, (h + 1) // 2, (w + 1) // 2).to(dt)
    elif c.op == "weight_std":
        # per-channel offsets for the standardisation to remove.  Two rows standardise to +-1 whatever they hold, and the gradient through that is
        # zero but for eps: there is nothing to compare a result with unless the spread is of the size of sqrt(eps), so there it is
        d["w"] = [rn(*s) * (2e-6 if _fan(s) == 2 else 0.05) + rn(s[-1]) * 0.3 for s in c.shape]
        d["gout"] = [rn(*s) for s in c.shape]
    elif c.op == "softmax_xent":
        n, k = c.shape
        z = rn(n, k) * 3.0
        z[n // 2] = torch.linspace(-80.0, 80.0, k)[torch.randperm(k, generator=g)]          # a +-80 spread
        target = torch.randint(0, k, (n,), generator=g)
        target[::2] = z[::2].argmax(dim=1)                                                    # every other row is a hit
        y = torch.eye(k)[target]
        if a["soft"]:
            y = 0.9 * y + 0.1 * torch.softmax(rn(n, k), dim=1)
            y[n // 3] *= 0.9                                                                  # a row that sums to 0.9 ...
            if n > 1:
                y[n - 1] = 0.0                                                                # ... and one that sums to 0 (its argmax: column 0)
        # two equal maxima in the logits of row 0: the first wins, as tf.argmax -- a hit when the label sits on the first, a miss on the second
        if a["ties"]:
            z[0, 7], z[0, 40] = 90.0, 90.0
            if n > 2:
                z[2, 7], z[2, 40] = 90.0, 90.0
                y[2] = torch.eye(k)[40]
            y[0] = torch.eye(k)[7] * (0.9 if a["soft"] else 1.0)
        d["logits"], d["labels"] = z, y
    elif c.op == "momentum":
        n = c.shape[0]
        d["p"], d["g"], d["accum"] = rn(n), rn(n), 0.5 * rn(n)
        d.update(wd=1e-2, lr=0.05, momentum=0.9)
    return d


def gn_relu_bwd_closed(x, gamma, beta, gy, groups, eps=EPS):
    """Group norm + ReLU backward written out (float64): (dx, dgamma, dbeta, pre).  With xh = (x - mean) rstd per (image, group),
    g' = gy [gamma xh + beta > 0] and a = gamma g':  dbeta = sum g', dgamma = sum g' xh, dx = rstd (a - mean_g(a) - xh mean_g(a xh))."""
    n, c, h, w = x.shape
    st = RR.group_stats(x, groups, eps)
    mean = st[..., 0].repeat_interleave(c // groups, dim=1).view(n, c, 1, 1)
    rstd = st[..., 1].repeat_interleave(c // groups, dim=1).view(n, c, 1, 1)
    xh = (x - mean) * rstd
    pre = xh * gamma.view(1, c, 1, 1) + beta.view(1, c, 1, 1)
    gp = torch.where(pre > 0, gy, torch.zeros_like(gy))
    a = gp * gamma.view(1, c, 1, 1)

    def group_mean(t):
        return t.reshape(n, groups, -1).mean(dim=2).repeat_interleave(c // groups, dim=1).view(n, c, 1, 1)
    dx = rstd * (a - group_mean(a) - xh * group_mean(a * xh))
    return dx, (gp * xh).sum(dim=(0, 2, 3)), gp.sum(dim=(0, 2, 3)), pre


def gn_bwd_reference(c, d):
    """(dx, dgamma, dbeta, pre, up) of a gn_bwd / gn_head_bwd case in float64, without addend and accumulate; up: the upstream gradient per element."""
    n, ch, h, w, G = c.shape
    x, gamma, beta = d["x"].double(), d["gamma"].double(), d["beta"].double()
    up = d["gy"].double() if c.op == "gn_bwd" else (d["gf"].double() / (h * w)).view(n, ch, 1, 1).expand(n, ch, h, w)
    if c.args.get("large"):
        return gn_relu_bwd_closed(x, gamma, beta, up, G) + (up,)
    xr, gr, br = (t.clone().requires_grad_(True) for t in (x, gamma, beta))
    pre = RR.group_norm(xr, gr, br, G)
    if c.op == "gn_bwd":
        torch.relu(pre).backward(up)
    else:
        torch.relu(pre).mean(dim=(2, 3)).backward(d["gf"].double())
    return xr.grad, gr.grad, br.grad, pre.detach(), up


def undecided(pre):
    """Elements whose ReLU decision is within rounding of zero (float64 pre-activation)."""
    return pre.abs() < UNDECIDED * pre.abs().max()


def undecided_share(c, d=None):
    d = inputs(c) if d is None else d
    return float(undecided(gn_bwd_reference(c, d)[3]).double().mean())


# a reference entry: how one result is held against float64
Exact = namedtuple("Exact", "ref")                       # the bits of ref in the result's dtype
Gemm = namedtuple("Gemm", "ref K mag absref")            # (K + 2) 2^-24 mag element by element; absref: |ref| of the bf16 term (a pooled one for the pool)
Ceil = namedtuple("Ceil", "ref family keep")             # family ceiling of max |ref|; keep: the elements compared (None: all)


def _gemm(ref, K, mag, absref=None):
    return Gemm(ref, K, mag, ref.abs() if absref is None else absref)


def _ceil(ref, family, keep=None):
    return Ceil(ref, family, keep)


def _grad(fn, shape, gy):
    """The gradient of the linear map fn at a leaf of `shape`, against gy."""
    leaf = torch.zeros(shape, dtype=torch.float64, requires_grad=True)
    return torch.autograd.grad(fn(leaf), leaf, gy)[0]


def first_argmax(t):
    return torch.from_numpy(np.argmax(t.numpy(), axis=1))   # (numpy: the first of equal maxima)


def reference(c, d):
    """name -> reference entry, float64 from the definition of the operation on the operands as stored."""
    a = c.args
    if c.op == "gn_stats":
        G = c.shape[4]
        s, out = d["x"], {}
        if a["addend"]:   # the stored sum: one IEEE add in fp32, rounded to the dtype
            s = (d["x"].float() + d["addend"].float()).to(d["x"].dtype)
            out["sum"] = Exact(s)
        st = RR.group_stats(s.double(), G)
        out["mean"], out["rstd"] = _ceil(st[..., 0], "gn_mean"), _ceil(st[..., 1], "gn_rstd")
        return out
    if c.op in ("gn_apply", "gn_head"):
        n, ch, h, w, G = c.shape
        st = d["stats"].double()
        mean = st[..., 0].repeat_interleave(ch // G, dim=1).view(n, ch, 1, 1)
        rstd = st[..., 1].repeat_interleave(ch // G, dim=1).view(n, ch, 1, 1)
        y = (d["x"].double() - mean) * rstd * d["gamma"].double().view(1, ch, 1, 1) + d["beta"].double().view(1, ch, 1, 1)
        if c.op == "gn_head":
            return {"features": _ceil(torch.relu(y).mean(dim=(2, 3)), "gn_head")}
        return {"y": _ceil(torch.relu(y) if a["relu"] else y, "gn_apply")}
    if c.op in ("gn_bwd", "gn_head_bwd"):
        dx, dgamma, dbeta, pre, up = gn_bwd_reference(c, d)
        und = undecided(pre)
        if a.get("addend"):
            dx = dx + d["addend"].double()
        if a["accumulate"]:
            dgamma, dbeta = dgamma + d["dgamma0"].double(), dbeta + d["dbeta0"].double()
        return {"dx": _ceil(dx, "gn_bwd_dx", keep=~und), "dgamma": _ceil(dgamma, "gn_bwd_dgamma"), "dbeta": _ceil(dbeta, "gn_bwd_dbeta")}
    if c.op.startswith("conv1x1"):
        ci, co, stride, n, h, w = c.shape
        wt = d["w"].double()
        if c.op == "conv1x1_fwd":
            return {"y": _gemm(RR.conv2d(d["x"].double(), wt, None, stride), ci, RR.conv2d(d["x"].double().abs(), wt.abs(), None, stride))}
        gy = d["gy"].double()
        if c.op == "conv1x1_bwd_data":
            ref = _grad(lambda x: RR.conv2d(x, wt, None, stride), (n, ci, h, w), gy)
            mag = _grad(lambda x: RR.conv2d(x, wt.abs(), None, stride), (n, ci, h, w), gy.abs())
            if a["out"]:
                ref, mag = ref + d["out0"].double(), mag + d["out0"].double().abs()
            return {"gx": _gemm(ref, co, mag)}
        x = d["x"].double()
        ref = _grad(lambda v: RR.conv2d(x, v, None, stride), (1, 1, ci, co), gy)
        mag = _grad(lambda v: RR.conv2d(x.abs(), v, None, stride), (1, 1, ci, co), gy.abs())
        if a["out"]:
            ref, mag = ref + d["out0"].double(), mag + d["out0"].double().abs()
        return {"gw": _gemm(ref, n * (h // stride) * (w // stride), mag)}
    if c.op == "stem_pool":
        x, wt = d["x"].double(), d["w"].double()
        b = d["bias"].double() if a["bias"] else None
        stem = RR.conv2d(x, wt, b, 2)
        mag = RR.conv2d(x.abs(), wt.abs(), None if b is None else b.abs(), 2)
        out = {"stem": _gemm(stem, 98, mag)}
        if a["want_pool"]:   # |max a_i - max b_i| <= max |a_i - b_i|: the window's largest bound
            out["pool"] = _gemm(RR.max_pool(stem), 98, RR.max_pool(mag), RR.max_pool(stem.abs()))
        return out
    if c.op == "stem_wgrad":
        n, h, w = c.shape
        x, gs = d["x"].double(), d["gstem"].double()
        gw = _grad(lambda v: RR.conv2d(x, v, None, 2), (7, 7, 2, 64), gs)
        mw = _grad(lambda v: RR.conv2d(x.abs(), v, None, 2), (7, 7, 2, 64), gs.abs())
        gb, mb = gs.sum(dim=(0, 2, 3)), gs.abs().sum(dim=(0, 2, 3))
        if a["out"]:
            gw, mw, gb, mb = gw + d["gw0"].double(), mw + d["gw0"].double().abs(), gb + d["gb0"].double(), mb + d["gb0"].double().abs()
        K = n * (h // 2) * (w // 2)
        return {"gw": _gemm(gw, K, mw), "gb": _gemm(gb, K, mb)}
    if c.op == "max_pool":
        return {"y": Exact(RR.max_pool(d["x"].float()))}
    if c.op == "max_pool_bwd":   # a float64 sum of the stored gradients of the (at most 4) windows an element is the first maximum of
        xr = d["x"].double().requires_grad_(True)
        RR.max_pool(xr).backward(d["gy"].double())
        return {"gx": _ceil(xr.grad, "max_pool_bwd")}
    if c.op == "weight_std":
        out = {}
        for i, (w, go) in enumerate(zip(d["w"], d["gout"])):
            wr = w.double().requires_grad_(True)
            std = RR.weight_standardization(wr)
            std.backward(go.double())
            var = ((w.double() - w.double().mean(dim=(0, 1, 2), keepdim=True)) ** 2).mean(dim=(0, 1, 2))
            out[f"out{i}"], out[f"rstd{i}"], out[f"gw{i}"] = _ceil(std.detach(), "ws_out"), _ceil(1.0 / torch.sqrt(var + EPS), "ws_rstd"), _ceil(wr.grad, "ws_bwd")
        return out
    if c.op == "softmax_xent":
        z, y = d["logits"].double().requires_grad_(True), d["labels"].double()
        loss = -(torch.log_softmax(z, dim=1) * y).sum(dim=1).mean()
        loss.backward()
        out = {"loss": _ceil(loss.detach().reshape(1), "xent_loss"),
               "correct": Exact((first_argmax(d["logits"]) == first_argmax(d["labels"])).sum().to(torch.int32).reshape(1))}
        if a["want_grad"]:
            out["dlogits"] = _ceil(z.grad, "xent_dlogits")
        return out
    if c.op == "momentum":
        p, g, acc = (d[k].double().numpy() for k in ("p", "g", "accum"))
        lo, hi = a["lo"], a["hi"]
        g = g.copy()
        l2 = 0.5 * float((p[lo:hi] ** 2).sum())
        g[lo:hi] += np.float64(np.float32(d["wd"])) * p[lo:hi]
        lr, mom = np.float64(np.float32(d["lr"])), np.float64(np.float32(d["momentum"]))
        acc = mom * acc + g
        p = p - (lr * g + lr * mom * acc if a["nesterov"] else lr * acc)
        out = {"p": _ceil(torch.from_numpy(p), "momentum_p"), "accum": _ceil(torch.from_numpy(acc), "momentum_accum"),
               # the gradient buffer afterwards: cleared, or (zero_grad=False: the kernel stores nothing back) the bits it came with
               "g": Exact(torch.zeros_like(d["g"]) if a["zero_grad"] else d["g"])}
        if a["want_l2"]:
            out["l2"] = _ceil(torch.tensor([l2], dtype=torch.float64), "momentum_l2")
        return out
    raise AssertionError(c.op)


def zero_masks(c, d):
    """name -> a boolean mask of result elements that must be exactly zero."""
    a = c.args
    if c.op == "conv1x1_bwd_data" and c.shape[2] == 2 and not a["out"]:
        ci, co, stride, n, h, w = c.shape
        m = torch.ones(n, ci, h, w, dtype=torch.bool)
        m[:, :, ::2, ::2] = False
        return {"gx": m}
    return {}


# ------------------------------------------------------------------------------------------------------------------------------ the device
def _dev(t):
    t = t.to("cuda")
    return t.contiguous(memory_format=torch.channels_last) if t.dim() == 4 else t.contiguous()


def _flat(t):
    """A weight or an fp32 buffer: contiguous as it is (an HWIO weight is 4-D and not an activation)."""
    return t.to("cuda").contiguous()


def _gn_bwd_direct(K, c, x, stats, gamma, beta, up, addend, dgamma, dbeta):
    """The backward entry points with accumulate = 1, which no wrapper passes: dgamma / dbeta are added into."""
    n, ch, h, w, G = c.shape
    dx = torch.empty_like(x)
    ws = torch.empty(max(K.lib.gs_group_norm_bwd_workspace_bytes(n, h * w, ch, G), 256), dtype=torch.uint8, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    tail = (dx.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), n, h * w, ch, G, 1, c.dtype, ws.data_ptr(), ws.numel(), stream)
    if c.op == "gn_bwd":
        rc = K.lib.gs_group_norm_relu_bwd(x.data_ptr(), stats.data_ptr(), gamma.data_ptr(), beta.data_ptr(), up.data_ptr(),
                                          None if addend is None else addend.data_ptr(), *tail)
    else:
        rc = K.lib.gs_group_norm_relu_mean_bwd(x.data_ptr(), stats.data_ptr(), gamma.data_ptr(), beta.data_ptr(), up.data_ptr(), *tail)
    assert rc == 0, (rc, K.lib.gs_last_error())
    return dx, dgamma, dbeta


def run(K, c, d):
    """The case through its public entry point (gansynth_amd.kernels): name -> result tensor."""
    a = c.args
    if c.op == "gn_stats":
        G = c.shape[4]
        stats, s = K.group_norm_stats(_dev(d["x"]), G, EPS, addend=_dev(d["addend"]) if a["addend"] else None)
        out = {"mean": stats[..., 0], "rstd": stats[..., 1]}
        if a["addend"]:
            out["sum"] = s
        return out
    if c.op == "gn_apply":
        return {"y": K.group_norm_apply(_dev(d["x"]), _dev(d["stats"]), _dev(d["gamma"]), _dev(d["beta"]), relu=bool(a["relu"]))}
    if c.op == "gn_head":
        return {"features": K.group_norm_relu_mean(_dev(d["x"]), _dev(d["stats"]), _dev(d["gamma"]), _dev(d["beta"]))}
    if c.op in ("gn_bwd", "gn_head_bwd"):
        x, stats, gamma, beta = _dev(d["x"]), _dev(d["stats"]), _dev(d["gamma"]), _dev(d["beta"])
        up = _dev(d["gy"] if c.op == "gn_bwd" else d["gf"])
        addend = _dev(d["addend"]) if a.get("addend") else None
        if a["accumulate"]:
            dx, dgamma, dbeta = _gn_bwd_direct(K, c, x, stats, gamma, beta, up, addend, _dev(d["dgamma0"].clone()), _dev(d["dbeta0"].clone()))
        elif c.op == "gn_bwd":
            buf = torch.full((2, c.shape[1]), 7.0, device="cuda")   # dgamma= / dbeta= buffers: written, not added into
            dx, dgamma, dbeta = K.group_norm_relu_bwd(x, stats, gamma, beta, up, addend=addend, dgamma=buf[0], dbeta=buf[1])
        else:
            buf = torch.full((2, c.shape[1]), 7.0, device="cuda")
            dx, dgamma, dbeta = K.group_norm_relu_mean_bwd(x, stats, gamma, beta, up, dgamma=buf[0], dbeta=buf[1])
        return {"dx": dx, "dgamma": dgamma, "dbeta": dbeta}
    if c.op.startswith("conv1x1"):
        ci, co, stride, n, h, w = c.shape
        if c.op == "conv1x1_fwd":
            return {"y": K.conv1x1_fwd(_dev(d["x"]), _flat(d["w"]), stride)}
        if c.op == "conv1x1_bwd_data":
            out = _dev(d["out0"]).clone(memory_format=torch.preserve_format) if a["out"] else None
            return {"gx": K.conv1x1_bwd_data(_dev(d["gy"]), _flat(d["w"]), (n, ci, h, w), stride, out=out)}
        return {"gw": K.conv1x1_bwd_weight(_dev(d["x"]), _dev(d["gy"]), stride, out=_flat(d["out0"]).clone() if a["out"] else None)}
    if c.op == "stem_pool":
        stem, pool = K.resnet_stem_pool(_dev(d["x"]), _flat(d["w"]), _flat(d["bias"]) if a["bias"] else None, want_stem=True, want_pool=bool(a["want_pool"]))
        assert (pool is None) == (not a["want_pool"])
        return {"stem": stem, "pool": pool} if a["want_pool"] else {"stem": stem}
    if c.op == "stem_wgrad":
        gw0, gb0 = (_flat(d["gw0"]).clone(), _flat(d["gb0"]).clone()) if a["out"] else (None, None)
        gw, gb = K.resnet_stem_bwd_weight(_dev(d["x"]), _dev(d["gstem"]), out=gw0, bias_out=gb0)
        return {"gw": gw, "gb": gb}
    if c.op == "max_pool":
        return {"y": K.max_pool2d(_dev(d["x"]))}
    if c.op == "max_pool_bwd":
        return {"gx": K.max_pool2d_bwd(_dev(d["x"]), _dev(d["gy"]))}
    if c.op == "weight_std":
        rows = []
        for w, go in zip(d["w"], d["gout"]):
            wd = _flat(w)
            rows.append((wd, torch.empty_like(wd), torch.empty(w.shape[-1], device="cuda"), _flat(go).clone(), torch.empty_like(wd)))
        table = K.weight_standardize_table(rows)
        K.weight_standardize_batch(table, EPS)
        out = {}
        for i, (wd, o, rstd, gout, gw) in enumerate(rows):
            out[f"out{i}"], out[f"rstd{i}"], out[f"single{i}"] = o.clone(), rstd.clone(), K.weight_standardize(wd, EPS)
        K.weight_standardize_bwd_batch(table)
        for i, (wd, o, rstd, gout, gw) in enumerate(rows):
            out[f"gw{i}"], out[f"gout{i}"] = gw, gout
        return out
    if c.op == "softmax_xent":
        loss, dlogits, correct = K.softmax_xent(_dev(d["logits"]), _dev(d["labels"]), want_grad=bool(a["want_grad"]))
        assert (dlogits is None) == (not a["want_grad"])
        out = {"loss": loss, "correct": correct}
        if a["want_grad"]:
            out["dlogits"] = dlogits
        return out
    if c.op == "momentum":
        p, g, acc = _dev(d["p"]).clone(), _dev(d["g"]).clone(), _dev(d["accum"]).clone()
        l2 = K.momentum_tf_step(p, g, acc, d["lr"], d["momentum"], bool(a["nesterov"]), weight_decay=d["wd"], decay_range=(a["lo"], a["hi"]),
                                zero_grad=bool(a["zero_grad"]), want_l2=bool(a["want_l2"]))
        assert (l2 is None) == (not a["want_l2"])
        out = {"p": p, "accum": acc, "g": g}
        if a["want_l2"]:
            out["l2"] = l2
        return out
    raise AssertionError(c.op)


def within(got, entry):
    """(family or None, ratio = max error over max |ref|, ok) of one result against its reference entry."""
    g = got.detach().cpu()
    if isinstance(entry, Exact):
        ok = g.shape == entry.ref.shape and torch.equal(g, entry.ref.to(g.dtype))
        return None, 0.0 if ok else float("inf"), ok
    g, ref = g.double().reshape(entry.ref.shape), entry.ref.double()
    err = (g - ref).abs()
    top = float(ref.abs().max())
    bf16 = 2.0 ** -8 * (entry.absref if isinstance(entry, Gemm) else ref.abs()) if got.dtype == torch.bfloat16 else 0.0
    if isinstance(entry, Gemm):
        bound = (entry.K + 2) * 2.0 ** -24 * entry.mag + bf16
        return None, float(err.max()) / (top + 1e-300), bool((err <= bound).all())
    if top == 0.0:   # (fan_in = 1; an empty decayed range)
        return entry.family, 0.0, bool((g == 0).all())
    bound = CEILINGS[entry.family][2] * top + bf16
    if entry.keep is not None:
        err, bound = err[entry.keep], (bound[entry.keep] if torch.is_tensor(bound) else bound)
    return entry.family, float(err.max()) / top, bool((err <= bound).all())
