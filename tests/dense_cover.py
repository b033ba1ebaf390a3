"""The cases of the dense kernels (csrc/dense.hip) -- shared by tests/test_dense_cover_cpu.py and tests/test_dense_cover_gpu.py (a plain helper
module: no fixtures, no collection hooks).

KERNELS is the list of compiled instantiations as dense.hip's launchers spell them; a case is a layer, one of its three maps and what is asked of
it (bias, activation, accumulate, a channels-last input side, the GS_NO_DENSE_MFMA knob), together with the instantiation `key` it is there for
and, where a finalize launch follows, the ksplit that launch folds.  Which kernel a case runs is not decided here: both test files ask the library
(gs_dense_route, host arithmetic on the route the entry points read) and hold the answer against the case's key.  `route_py` is a restatement of
csrc/dense_route.h for the CPU test's sweep; `reference` is float64 on the operands as stored (activations rounded to bf16 for bf16, weights and
bias fp32).

Every result is held element by element to the bound of tests/cover_bounds.py (`bound`): K = in (forward), out (data gradient) or b (weight
gradient), e = 3 (+ 1 for a leaky-relu slope), u = 2^-24 throughout (dense.hip runs the f32 MFMA, a k-ordered fmaf chain, for bf16 as well); a bf16
result is rounded once, the weight gradients are fp32 results in both dtypes and take the fp32 rule.

Worst max error over max |ref| of the fp32 results measured on the MI355X over seeds 0 .. 11 of every case, knob unset and set together (1536
comparisons; tests/test_dense_cover_gpu.py prints the column: DENSE-COVER-WORST), the dense tests' ceiling and the ceiling held here (CEILINGS
below; the CPU test holds the two copies together):
    family            measured    suite   here
    fwd               1.6e-07     0.001   1e-05
    fwd_small         4.2e-07     0.001   1e-05
    fwd_fast          5.1e-07     0.001   1e-05
    fwd_mfma          2.5e-07     0.001   1e-05
    bwd_data          1.6e-07     0.001   1e-05
    bwd_data_wide     1.4e-07     0.001   1e-05
    bwd_data_fast     1.8e-07     0.001   1e-05
    bwd_data_mfma     7.3e-07     0.001   0.0001
    bwd_weight        2.9e-07     0.001   1e-05
    bwd_weight_fast   1.5e-07     0.001   1e-05
Beside it, worst bf16 ratio and worst err / bound (fp32 results, bf16 results) per family: fwd 3.3e-3, 0.02, 0.985; fwd_small 3.8e-3, 0.04, 0.980;
fwd_fast 3.6e-3, 0.05, 0.990; fwd_mfma 3.6e-3, 0.02, 0.978; bwd_data 3.3e-3, 0.04, 0.993; bwd_data_wide 2.8e-3, 0.01, 0.963; bwd_data_fast 3.6e-3,
0.02, 0.988; bwd_data_mfma 3.4e-3, 0.09, 0.993; bwd_weight (K = b <= 20) 0.32; bwd_weight_fast (K = 5) 0.40.
"""
import ctypes
from collections import namedtuple

import torch

from tests import cover_bounds as B
from tests import igemm_cover

F32, BF16 = 0, 1
DTYPE_NAMES = ("f32", "bf16")
TORCH_DTYPE = {F32: torch.float32, BF16: torch.bfloat16}
FWD_MAP, BWD_DATA_MAP, BWD_WEIGHT_MAP = range(3)                       # GS_DENSE_MAP_*
MAP_NAMES = ("fwd", "bwd_data", "bwd_weight")
FWD, FWD_SMALL, FWD_FAST, FWD_MFMA, FINALIZE, BWD_DATA, BWD_DATA_WIDE, BWD_DATA_FAST, BWD_DATA_MFMA, BWD_WEIGHT, BWD_WEIGHT_FAST = range(11)   # GS_DENSE_*
KERNEL_NAMES = ("fwd", "fwd_small", "fwd_fast", "fwd_mfma", "finalize", "bwd_data", "bwd_data_wide", "bwd_data_fast", "bwd_data_mfma", "bwd_weight",
                "bwd_weight_fast")
NONE, LRELU, TANH = 0, 1, 2                                            # GS_ACT_*
ACT_NAMES = ("none", "lrelu", "tanh")
ERR_ARG, ERR_UNSUPPORTED = -1, -3
# the dense tests' own ceilings (tests/test_kernels_gpu.py), of max |ref|: forward and data gradient by dtype, weight gradient (fp32 out) in both
TOLERANCE = {FWD_MAP: {F32: 1e-3, BF16: 2e-2}, BWD_DATA_MAP: {F32: 1e-3, BF16: 2e-2}, BWD_WEIGHT_MAP: {F32: 1e-3, BF16: 1e-3}}
# kernel -> (worst fp32-result ratio measured on the MI355X, the dense tests' ceiling, the ceiling held here: cover_bounds.ceiling_rule): the
# docstring's table.  The weight gradients of bf16 operands are fp32 results and count with their kernel.
CEILINGS = {
    "fwd":               (1.6e-07, 0.001, 1e-05),
    "fwd_small":         (4.2e-07, 0.001, 1e-05),
    "fwd_fast":          (5.1e-07, 0.001, 1e-05),
    "fwd_mfma":          (2.5e-07, 0.001, 1e-05),
    "bwd_data":          (1.6e-07, 0.001, 1e-05),
    "bwd_data_wide":     (1.4e-07, 0.001, 1e-05),
    "bwd_data_fast":     (1.8e-07, 0.001, 1e-05),
    "bwd_data_mfma":     (7.3e-07, 0.001, 0.0001),
    "bwd_weight":        (2.9e-07, 0.001, 1e-05),
    "bwd_weight_fast":   (1.5e-07, 0.001, 1e-05),
}
ROUTE_FIELDS = ("kernel", "FB", "WPR", "step", "passes", "grid_x", "grid_y", "ksplit", "ipb", "finalize", "ws_bytes")
DENSE_BT, DENSE_WR = 16, 16

Key = namedtuple("Key", "kernel dtype FB WPR")   # one compiled instantiation
Route = namedtuple("Route", ROUTE_FIELDS)
# (b, in, out): the layer; c, hw != 0: its input side channels-last; fin: the ksplit of the finalize launch that follows (0: none follows)
Case = namedtuple("Case", "key map b inp out c hw act bias accumulate no_mfma fin")


def _key(kernel, dtype, FB=0, WPR=0):
    return Key(kernel, dtype, FB, WPR)


KERNELS = (
    [_key(k, d) for d in (F32, BF16) for k in (FWD, FWD_SMALL, FWD_MFMA, FINALIZE, BWD_DATA, BWD_DATA_WIDE, BWD_DATA_MFMA, BWD_WEIGHT, BWD_WEIGHT_FAST)]
    + [_key(FWD_FAST, d, FB=fb) for d in (F32, BF16) for fb in (8, 16, 24)]
    + [_key(BWD_DATA_FAST, d, FB=fb, WPR=wpr) for d in (F32, BF16) for wpr in (1, 4) for fb in (8, 16, 24)]
)
assert len(KERNELS) == len(set(KERNELS)) == 36


def key_id(k):
    return "-".join([KERNEL_NAMES[k.kernel], DTYPE_NAMES[k.dtype]] + [f"{f}{v}" for f, v in zip(Key._fields[2:], k[2:]) if v])


def case_id(c):
    extra = [ACT_NAMES[c.act]] + (["bias"] if c.bias else []) + (["accumulate"] if c.accumulate else []) + (["no_mfma"] if c.no_mfma else [])
    side = f"{c.c}x{c.hw}" if c.c else f"{c.inp}"
    return f"{key_id(c.key)} {MAP_NAMES[c.map]} {c.b}x{side}->{c.out} " + "+".join(extra)


def query(lib, map_, b, inp, out, c=0, hw=0, dtype=F32, no_mfma=-1):
    """gs_dense_route: a Route, or the negative code the map's entry point refuses the layer with.  no_mfma -1: this process's environment."""
    from gansynth_amd import _lib
    ints = (ctypes.c_int * _lib.DENSE_ROUTE_INTS)()
    rc = lib.gs_dense_route(_lib.GsDense(b, inp, out, c, hw, dtype, 1.0, None, 0), map_, no_mfma, ints)
    return rc if rc else Route(*ints[:10], (ints[10] & 0xFFFFFFFF) | (ints[11] << 32))


def route(lib, c, no_mfma=None):
    return query(lib, c.map, c.b, c.inp, c.out, c.c, c.hw, c.key.dtype, c.no_mfma if no_mfma is None else no_mfma)


def route_key(r, dtype):
    return Key(r.kernel, dtype, r.FB, r.WPR)


def case_keys(c):
    """The instantiations a case launches: its own and, where one follows, the finalize pass."""
    return {c.key} | ({_key(FINALIZE, c.key.dtype)} if c.fin else set())


# ------------------------------------------------------------------------------------------------------------- the route, restated
def _cdiv(a, b):
    return -(-a // b)


def _fast_rows(b):
    return 8 if b <= 8 else (16 if b <= 16 else 24)


def route_py(map_, b, inp, out, rc=0, rhw=0, no_mfma=0):
    """csrc/dense_route.h: dense_route, condition for condition: a Route or the error code."""
    if not (b > 0 and inp > 0 and out > 0) or not (rc == 0 or (rc > 0 and rhw > 0 and rc * rhw == inp)):
        return ERR_ARG
    if map_ == FWD_MAP:
        fast = inp % 4 == 0 and out % 32 == 0
        mfma = not no_mfma and inp >= 2048 and inp % 64 == 0 and out % 64 == 0 and out <= 1024
        if rc and not fast:
            return ERR_UNSUPPORTED
        if mfma:
            ks, ipb = inp // 64, 64
        elif fast:
            tiles = out // 32
            ks = max(1, min(1 if tiles >= 128 else _cdiv(512, tiles), max(inp // 128, 1)))
            ipb = (_cdiv(inp, ks) + 3) & ~3
            ks = _cdiv(inp, ipb)
        else:
            ks = max(1, min(max(1024 // _cdiv(out, 64), 1), max(inp // 32, 1)))
            ipb = _cdiv(inp, ks)
            ks = _cdiv(inp, ipb)
        ws = ks * b * out * 4
        if not rc and inp <= 1024 and out <= 256 and b <= 64:
            return Route(FWD_SMALL, 0, 0, b, 1, _cdiv(out, 64), b, 1, inp, 0, ws)
        if mfma:
            return Route(FWD_MFMA, 0, 0, b, 1, _cdiv((out // 64) * ks, 4), 1, ks, ipb, 1, ws)
        if fast:
            fb = _fast_rows(b)
            return Route(FWD_FAST, fb, 0, fb, _cdiv(b, fb), out // 32, ks, ks, ipb, int(ks > 1), ws)
        return Route(FWD, 0, 0, DENSE_BT, _cdiv(b, DENSE_BT), _cdiv(out, 64), ks, ks, ipb, 1, ws)
    if map_ == BWD_DATA_MAP:
        if rc and out % 256 != 0:
            return ERR_UNSUPPORTED
        if not no_mfma and inp >= 1024 and out % 16 == 0 and out <= 4096:
            return Route(BWD_DATA_MFMA, 0, 0, b, 1, _cdiv(_cdiv(inp, 16), 4), 1, 0, 0, 0, 0)
        if out % 256 == 0:
            fb, wpr = _fast_rows(b), (4 if inp <= 1024 and out >= 1024 else 1)
            return Route(BWD_DATA_FAST, fb, wpr, fb, _cdiv(b, fb), inp if wpr == 4 else _cdiv(inp, 4), 1, 0, 0, 0, 0)
        if out >= 2048:
            return Route(BWD_DATA_WIDE, 0, 0, DENSE_BT, _cdiv(b, DENSE_BT), inp, 1, 0, 0, 0, 0)
        return Route(BWD_DATA, 0, 0, DENSE_BT, _cdiv(b, DENSE_BT), _cdiv(inp, 4), 1, 0, 0, 0, 0)
    if map_ == BWD_WEIGHT_MAP:
        fast = out % 256 == 0 and b <= DENSE_BT
        if rc and not fast:
            return ERR_UNSUPPORTED
        if fast:
            return Route(BWD_WEIGHT_FAST, 0, 0, b, 1, out // 256, _cdiv(inp, DENSE_WR), 0, 0, 0, 0)
        return Route(BWD_WEIGHT, 0, 0, b, 1, _cdiv(inp * out, 256), 1, 0, 0, 0, 0)
    return ERR_ARG


# ---------------------------------------------------------------------------------------------------------------------------------- the cases
# the finalize pass walks its ksplit partials 8 at a time over 4 lanes (k, k + 4 per trip): at most 4 is the tail alone, 12 a trip and a tail,
# 16 and 32 whole trips
FIN_KINDS = {"tail only": (4,), "trip and tail": (12,), "whole trips": (16, 32)}


def _cases():
    out = []

    def add(key, map_, b, inp, o, c=0, hw=0, act=NONE, bias=False, accumulate=False, no_mfma=0, fin=0):
        assert not c or c * hw == inp
        out.append(Case(key, map_, b, inp, o, c, hw, act, bias, accumulate, no_mfma, fin))
    for d in (F32, BF16):
        # forward, small: one 64-row trip plus tail, the second column block ragged
        for act, bias in ((LRELU, True), (TANH, True), (NONE, False)):
            add(_key(FWD_SMALL, d), FWD_MAP, 5, 100, 70, act=act, bias=bias)
        # forward, generic: in % 4 != 0, two batch passes (16 + 4), ragged last K slice, finalize over 32 slices
        add(_key(FWD, d), FWD_MAP, 20, 1030, 70, fin=32)
        add(_key(FWD, d), FWD_MAP, 20, 1030, 70, act=LRELU, bias=True, fin=32)
        # forward, fast with a split: 4 slices with a ragged last one, every FB, a second pass (24 + 6); the row map; 12 slices
        for b in (5, 13, 24, 30):
            add(_key(FWD_FAST, d, FB=8 if b <= 8 else (16 if b <= 16 else 24)), FWD_MAP, b, 520, 288, act=LRELU, bias=True, fin=4)
        add(_key(FWD_FAST, d, FB=16), FWD_MAP, 13, 520, 288, c=8, hw=65, fin=4)
        add(_key(FWD_FAST, d, FB=8), FWD_MAP, 5, 1544, 288, act=TANH, bias=True, fin=12)
        # forward, fast without one: rows ragged against the 128-row stride, the epilogue in the kernel
        add(_key(FWD_FAST, d, FB=8), FWD_MAP, 5, 132, 4096, act=TANH, bias=True)
        add(_key(FWD_FAST, d, FB=8), FWD_MAP, 5, 132, 4096)
        # forward on the MFMA: plain; the row map wrapping inside a lane's 16-row run (c = 8) and the model's (c = 256).  With the knob set the
        # same shapes run the fast kernel with 16 slices
        for b in (5, 20):
            for c, hw in ((0, 0), (8, 256), (256, 8)):
                add(_key(FWD_MFMA, d), FWD_MAP, b, 2048, 64, c=c, hw=hw, act=LRELU, bias=True, fin=32)
                add(_key(FWD_FAST, d, FB=8 if b == 5 else 24), FWD_MAP, b, 2048, 64, c=c, hw=hw, act=LRELU, bias=True, no_mfma=1, fin=16)
        # data gradient on the MFMA: in % 16 != 0; the row map.  With the knob set: the generic kernel, the wave-per-row fast kernel
        for b in (5, 20):
            add(_key(BWD_DATA_MFMA, d), BWD_DATA_MAP, b, 1034, 48)
            add(_key(BWD_DATA, d), BWD_DATA_MAP, b, 1034, 48, no_mfma=1)
        add(_key(BWD_DATA_MFMA, d), BWD_DATA_MAP, 5, 1024, 256, c=4, hw=256)
        add(_key(BWD_DATA_FAST, d, FB=8, WPR=1), BWD_DATA_MAP, 5, 1024, 256, c=4, hw=256, no_mfma=1)
        # data gradient, fast: the block on one row (WPR 4) and a wave per row (WPR 1, `in` ragged against the 4 rows of a block), every FB
        for b in (5, 13, 24, 30):
            fb = 8 if b <= 8 else (16 if b <= 16 else 24)
            add(_key(BWD_DATA_FAST, d, FB=fb, WPR=4), BWD_DATA_MAP, b, 6, 1024)
            add(_key(BWD_DATA_FAST, d, FB=fb, WPR=1), BWD_DATA_MAP, b, 6, 256)
        add(_key(BWD_DATA_FAST, d, FB=16, WPR=1), BWD_DATA_MAP, 13, 6, 256, c=2, hw=3)
        add(_key(BWD_DATA_WIDE, d), BWD_DATA_MAP, 20, 5, 2056)
        add(_key(BWD_DATA, d), BWD_DATA_MAP, 20, 7, 70)
        # weight gradient: overwrite and accumulate into a non-zero buffer; the row map; the generic kernel's two 8-row trips plus tail, tail only
        for acc in (False, True):
            add(_key(BWD_WEIGHT_FAST, d), BWD_WEIGHT_MAP, 5, 20, 256, accumulate=acc)
            add(_key(BWD_WEIGHT_FAST, d), BWD_WEIGHT_MAP, 5, 20, 256, c=4, hw=5, accumulate=acc)
            add(_key(BWD_WEIGHT, d), BWD_WEIGHT_MAP, 20, 7, 70, accumulate=acc)
            add(_key(BWD_WEIGHT, d), BWD_WEIGHT_MAP, 5, 7, 70, accumulate=acc)
    return out


CASES = _cases()


def families():
    """(kernel template, dtype) of every GPU test, with its cases -- the finalize pass with the cases it rides on."""
    out = {}
    for c in CASES:
        for k in case_keys(c):
            out.setdefault((k.kernel, k.dtype), []).append(c)
    return out


def family_id(f):
    return f"{KERNEL_NAMES[f[0]]}-{DTYPE_NAMES[f[1]]}"


# --------------------------------------------------------------------------------------------------------------------- operands and reference
def _side(c):
    """The shape of the input side: [b, in], or the logical NCHW shape of the channels-last activation."""
    if not c.c:
        return c.b, c.inp
    h = next((f for f in range(2, c.hw) if c.hw % f == 0), 1)
    return c.b, c.c, h, c.hw // h


def inputs(c, seed=5):
    """The operands of a case as stored (CPU; activations rounded to the case's dtype): a dict with a, w, alpha and the optional bias, x, gw0."""
    g = torch.Generator().manual_seed(seed)
    dt = TORCH_DTYPE[c.key.dtype]
    d = {"w": torch.randn(c.inp, c.out, generator=g), "alpha": float((2.0 / c.inp) ** 0.5)}
    d["a"] = torch.randn(*(_side(c) if c.map != BWD_DATA_MAP else (c.b, c.out)), generator=g).to(dt)   # x, or gy of the data gradient
    if c.map == BWD_WEIGHT_MAP:
        d["gy"] = torch.randn(c.b, c.out, generator=g).to(dt)
        if c.accumulate:
            d["gw0"] = 0.5 * torch.randn(c.inp, c.out, generator=g)
    if c.bias:
        d["bias"] = 0.5 * torch.randn(c.out, generator=g)
    return d


def reference(c, d):
    a, w = d["a"].double(), d["w"].double()
    if c.map == FWD_MAP:   # (a 4-D activation: tf.layers.flatten of NCHW, column ch * hw + p)
        y = d["alpha"] * a.reshape(c.b, -1) @ w
        if c.bias:
            y = y + d["bias"].double()
        return torch.tanh(y) if c.act == TANH else (torch.where(y > 0, y, 0.2 * y) if c.act == LRELU else y)
    if c.map == BWD_DATA_MAP:
        return (d["alpha"] * a @ w.t()).reshape(_side(c))
    gw = d["alpha"] * a.reshape(c.b, -1).t() @ d["gy"].double()
    return gw + d["gw0"].double() if c.accumulate else gw


def _map(c, a, w, gy=None):
    """The map of the case without alpha, bias and accumulate, in the dtype of its operands."""
    if c.map == FWD_MAP:   # (a 4-D activation: tf.layers.flatten of NCHW, column ch * hw + p)
        return a.reshape(c.b, -1) @ w
    if c.map == BWD_DATA_MAP:
        return (a @ w.t()).reshape(_side(c))
    return a.reshape(c.b, -1).t() @ gy


def restated(c, d):
    """An honest kernel: the map in fp32 (torch on the CPU) on the operands as stored, alpha, bias, activation and accumulate behind it in fp32,
    one store in the result's dtype (fp32 for a weight gradient)."""
    y = d["alpha"] * _map(c, d["a"].float(), d["w"].float(), d["gy"].float() if c.map == BWD_WEIGHT_MAP else None)
    if c.map == BWD_WEIGHT_MAP:
        return y + d["gw0"] if c.accumulate else y
    if c.bias:
        y = y + d["bias"].float()
    y = torch.tanh(y) if c.act == TANH else (torch.where(y > 0, y, 0.2 * y) if c.act == LRELU else y)
    return y.to(TORCH_DTYPE[c.key.dtype])


def mag(c, d):
    """cover_bounds' mag: |alpha| map(|a|, |w|) + |bias| + |gw0| in fp32 on the CPU."""
    m = abs(d["alpha"]) * _map(c, d["a"].float().abs(), d["w"].float().abs(), d["gy"].float().abs() if c.map == BWD_WEIGHT_MAP else None)
    if c.bias:
        m = m + d["bias"].float().abs()
    return m + d["gw0"].float().abs() if c.accumulate else m


def products(c):
    """K: what an element of the map sums over -- in, out or b."""
    return (c.inp, c.out, c.b)[c.map]


def family(c):
    return KERNEL_NAMES[c.key.kernel]


def roundings(c):
    """bf16 results are rounded once (bias and activation ride in the kernel or in the finalize pass, on fp32 partials); weight gradients are fp32."""
    return 1 if (c.key.dtype == BF16 and c.map != BWD_WEIGHT_MAP) else 0


def bound(c, ref, m):
    """The element-wise bound of the case's result (tests/cover_bounds.py).  dense.hip runs the f32 MFMA for bf16 as well: u = 2^-24 throughout."""
    return B.bound(ref, m, products(c), B.E_BASE + int(c.act == LRELU), CEILINGS[family(c)][2], roundings=roundings(c), tanh_fwd=c.act == TANH)


def macs(c):
    return c.b * c.inp * c.out


def run(K, c, d):
    """The case through its public entry point (gansynth_amd.kernels.HipKernels): the result tensor."""
    def dev(t):
        t = t.to("cuda")
        return t.contiguous(memory_format=torch.channels_last) if t.dim() == 4 else t
    a, w = dev(d["a"]), dev(d["w"])
    if c.map == FWD_MAP:
        return K.dense_fwd_bias_act(a, w, dev(d["bias"]) if c.bias else None, d["alpha"], c.act)
    if c.map == BWD_DATA_MAP:
        return K.dense_bwd_data_nhwc(a, w, _side(c), d["alpha"]) if c.c else K.dense_bwd_data(a, w, d["alpha"])
    gw0 = dev(d["gw0"].clone()) if c.accumulate else None
    return (K.dense_bwd_weight_nhwc if c.c else K.dense_bwd_weight)(a, dev(d["gy"]), d["alpha"], out=gw0)


def ratio(got, ref):
    return igemm_cover.ratio(got, ref)
