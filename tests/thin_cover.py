"""The cases of the VALU convs (csrc/conv_thin.hip) -- shared by tests/test_thin_cover_cpu.py and tests/test_thin_cover_gpu.py (a plain helper
module: no fixtures, no collection hooks).

KERNELS is the list of compiled instantiations as conv_thin.hip's launcher spells them; a case is a layer, one of its maps and what is asked of
it (bias, activation, mask, the norm's backward), together with the instantiation `key` it is there for.  Which kernel a case runs is not
decided here: both test files ask the library (gs_conv_thin_route, host arithmetic on the route the entry points read) and hold the answer
against the case's key.  `reference` is float64 on the operands as stored (activations rounded to bf16 for bf16; the thin kernels read their
weights and bias as fp32): the conv by its definition, bias, exact tanh / leaky relu, the mask's derivative from the given mask values and, for
EXPAND_PNBWD, the formula of the kernel's comment.

Every EXPAND and REDUCE case carries its own pixel count (pixels_for): the smallest of a fixed list at which a grid capped at 2 blocks makes at
least one full four-pass trip and at least one tail pass, and the last pass is ragged.  Compiled but out of reach of every entry point (and so
of the GPU test): thin_expand_kernel<.., ACT != none, MASKED> -- gs_conv_fwd_mask asks for no activation behind the conv.

Every result is held element by element to the bound of tests/cover_bounds.py (`bound`): K = ks^2 contracted channels (4 x where the transposed
walk reaches an element with at most 2 x 2 taps), e = 3 (+ 1 for a leaky-relu slope or mask factor, + 2 for a tanh mask), the masks operands of
`mag`; a bf16 result is rounded once, twice where the route leaves a pass behind the kernel (`roundings`: only masks are left so).  EXPAND_PNBWD's
reference is a composite: its bound is the ceiling part alone, plus the bf16 term.

Worst max error over max |ref| of the fp32 results measured on the MI355X over seeds 0 .. 11 of every case, default caps and caps of 2 together
(4584 comparisons; tests/test_thin_cover_gpu.py prints the column: THIN-COVER-WORST), the suite's ceiling and the ceiling held here (CEILINGS below;
the CPU test holds the two copies together):
    family            measured    suite   here
    expand            3.0e-07     0.001   1e-05
    reduce            5.1e-07     0.001   1e-05
    expand_pnbwd      2.2e-07     0.001   1e-05
    single3           2.6e-07     0.001   1e-05
    single            2.3e-07     0.001   1e-05
    direct            4.4e-07     0.001   1e-05
Beside it, worst bf16 ratio and worst err / bound (fp32 results, bf16 results) per family: expand 3.7e-3, 0.58, 0.996; reduce 4.1e-3, 0.13, 0.993;
expand_pnbwd 3.7e-3, 0.02, 0.991; single3 3.0e-3, 0.03, 0.969; single 3.5e-3, 0.02, 0.967; direct 3.4e-3, 0.36, 0.992.

What the bound found: the direct and single kernels used to leave bias and activation to a pass behind them, which for bf16 added the bias to a sum
already rounded to bf16.  Where sum and bias cancel, that rounding is many times the result's own: 93 of the 12-seed comparisons of the nine bf16
cases with a bias were outside (worst err / bound 241 direct, 20 single3, 9.5 single) while their max-norm ratios, 1.4e-3 .. 6.6e-3, passed the old
1e-2.  Both steps now ride in those kernels on the fp32 sum (conv_thin.hip: bias_act_rt; the fp32 cases measure what they measured before).
"""
import ctypes
import itertools
from collections import namedtuple

import torch

from tests import cover_bounds as B
from tests import igemm_cover

F32, BF16 = 0, 1
DTYPE_NAMES = ("f32", "bf16")
TORCH_DTYPE = {F32: torch.float32, BF16: torch.bfloat16}
EXPAND, REDUCE, EXPAND_PNBWD, SINGLE3, SINGLE, DIRECT = range(6)      # GS_THIN_* kernels
KERNEL_NAMES = ("expand", "reduce", "expand_pnbwd", "single3", "single", "direct")
PLAIN, FWD_MASK, BWD_PNBWD = range(3)                                  # GS_THIN_* forms
NONE, LRELU, TANH = 0, 1, 2                                            # GS_ACT_*
ACT_NAMES = ("none", "lrelu", "tanh")
S1, S2, T2 = 0, 1, 2
MODE_NAMES = ("S1", "S2", "T2")
CONV_FWD, CONV_BWD_DATA = 0, 1
TOLERANCE = igemm_cover.TOLERANCE   # the suite's ceilings for conv forward and data gradients: 1e-3 fp32, 1e-2 bf16 of max |ref|
# family -> (worst fp32 ratio measured on the MI355X, the suite's ceiling, the ceiling held here: cover_bounds.ceiling_rule): the docstring's table
CEILINGS = {
    "expand":            (3.0e-07, 0.001, 1e-05),
    "reduce":            (5.1e-07, 0.001, 1e-05),
    "expand_pnbwd":      (2.2e-07, 0.001, 1e-05),
    "single3":           (2.6e-07, 0.001, 1e-05),
    "single":            (2.3e-07, 0.001, 1e-05),
    "direct":            (4.4e-07, 0.001, 1e-05),
}
CAPPED = (2, 2)                     # both grid caps of the capped runs
EPS = 1e-8
ROUTE_FIELDS = ("kernel", "C", "ACT", "MASKED", "LC", "OCV", "VEC", "grid", "ppb", "trips", "tails", "epilogue_fused", "mask_fused", "bits_fused")

Key = namedtuple("Key", "kernel dtype C ACT MASKED LC OCV VEC")   # one compiled instantiation (the first seven ints of the route, and the dtype)
Route = namedtuple("Route", ROUTE_FIELDS)
# call: fwd / fwd_t (transposed layer) / fwd_mask / bwd_data / bwd_data_t / pnbwd; (n, h, w, ci, co, ks, stride): the LAYER, forward labelling
Case = namedtuple("Case", "key call n h w ci co ks stride act bias mask_act addend")


def _key(kernel, dtype, C=0, ACT=0, MASKED=0, LC=0, OCV=0, VEC=0):
    return Key(kernel, dtype, C, ACT, MASKED, LC, OCV, VEC)


KERNELS = (
    [_key(EXPAND, d, C=ic, ACT=a, MASKED=m) for d in (F32, BF16) for ic in (1, 2, 3, 4) for a in (NONE, LRELU, TANH) for m in (0, 1)]
    + [_key(REDUCE, d, C=oc, ACT=a, LC=lc) for d in (F32, BF16) for oc in (1, 2, 3, 4) for a in (NONE, LRELU, TANH) for lc in (4, 8, 0)]
    + [_key(EXPAND_PNBWD, d, C=ic) for d in (F32, BF16) for ic in (1, 2, 3, 4)]
    + [_key(SINGLE3, d) for d in (F32, BF16)]
    + [_key(SINGLE, d) for d in (F32, BF16)]
    + [_key(DIRECT, d, OCV=ocv, VEC=vec) for d in (F32, BF16) for ocv in (4, 2, 1) for vec in (4, 1)]
)
assert len(KERNELS) == len(set(KERNELS)) == 144


def key_id(k):
    return "-".join([KERNEL_NAMES[k.kernel], DTYPE_NAMES[k.dtype]] + [f"{f}{v}" for f, v in zip(Key._fields[2:], k[2:]) if v])


def case_id(c):
    extra = [ACT_NAMES[c.act]] + (["bias"] if c.bias else []) + ([f"mask-{ACT_NAMES[c.mask_act]}"] if c.mask_act else []) + (["addend"] if c.addend else [])
    return f"{key_id(c.key)} {c.call} {c.n}x{c.h}x{c.w} {c.ci}->{c.co} k{c.ks}s{c.stride} " + "+".join(extra)


def layer(c):
    """(GsConv fields n, h, w, ci, co, ks, stride, transposed), map, form of a case."""
    transposed = 1 if c.call in ("fwd_t", "bwd_data_t") else 0
    map_ = CONV_FWD if c.call in ("fwd", "fwd_t", "fwd_mask") else CONV_BWD_DATA
    form = FWD_MASK if c.call == "fwd_mask" else (BWD_PNBWD if c.call == "pnbwd" else PLAIN)
    return (c.n, c.h, c.w, c.ci, c.co, c.ks, c.stride, transposed), map_, form


def mode(c):
    """The kernel-role mode of a case (conv_api.hip: conv_role)."""
    fwd = c.call in ("fwd", "fwd_t", "fwd_mask")
    if c.call in ("fwd_t", "bwd_data_t"):
        return T2 if fwd else S2
    return S1 if c.stride == 1 else (S2 if fwd else T2)


def query(lib, desc, dtype, map_, form, act, has_bias, mask_act, want_bits, caps=None):
    """gs_conv_thin_route for a layer: a Route, or None when the call belongs to the implicit GEMM.  caps None: this process's environment."""
    from gansynth_amd import _lib
    out = (ctypes.c_int * _lib.THIN_ROUTE_INTS)()
    conv = _lib.GsConv(*desc, dtype, 0, 1.0, None, 0)
    rc = lib.gs_conv_thin_route(conv, map_, form, act, int(has_bias), mask_act, int(want_bits), None if caps is None else (ctypes.c_int * 2)(*caps), out)
    assert rc == 0, (rc, lib.gs_last_error())
    return None if out[0] < 0 else Route(*out)


def route(lib, c, caps=None, want_bits=False):
    desc, map_, form = layer(c)
    return query(lib, desc, c.key.dtype, map_, form, c.act, c.bias, c.mask_act, want_bits, caps)


def route_key(r, dtype):
    return Key(r.kernel, dtype, *r[1:7])


# ---------------------------------------------------------------------------------------------------------------------------------- the cases
_PIXELS = sorted(((n * h * w, (n, h, w)) for n in (1, 2) for h in (3, 5, 9, 11) for w in (7, 23, 33, 35, 37, 121)))


def pixels_for(ppb):
    """(n, h, w) with the fewest pixels such that two blocks of ppb pixels per pass make >= 1 four-pass trip and >= 1 tail pass, the last one ragged."""
    for p, dims in _PIXELS:
        npass = -(-p // (2 * ppb))
        if npass >= 5 and npass % 4 != 0 and p % ppb != 0:
            return dims
    raise AssertionError(ppb)


def _wn(d):
    return 4 if d == F32 else 8


def _cases():
    out = []

    def add(key, call, dims, ci, co, ks=1, stride=1, act=NONE, bias=False, mask_act=NONE, addend=False):
        out.append(Case(key, call, *dims, ci, co, ks, stride, act, bias, mask_act, addend))
    for d in (F32, BF16):
        wn = _wn(d)
        # EXPAND: few -> many channels.  Four lanes per pixel (the colour block at 32 bf16 channels): every IC x ACT with a bias; masked; no bias
        px = pixels_for(64)
        for ic, a in itertools.product((1, 2, 3, 4), (NONE, LRELU, TANH)):
            add(_key(EXPAND, d, C=ic, ACT=a), "fwd", px, ic, 4 * wn, act=a, bias=True)
        for ic, ma in ((1, TANH), (2, LRELU), (3, TANH), (4, LRELU)):
            add(_key(EXPAND, d, C=ic, MASKED=1), "fwd_mask", px, ic, 4 * wn, mask_act=ma)
        add(_key(EXPAND, d, C=2), "fwd", px, 2, 4 * wn)
        for groups in (1, 2, 8, 64, 128):   # other lane counts per pixel; as the data gradient of the colour layer on the other side, with a mask pass behind it
            add(_key(EXPAND, d, C=2, ACT=LRELU), "fwd", pixels_for(256 // groups), 2, groups * wn, act=LRELU, bias=True)
        add(_key(EXPAND, d, C=2), "bwd_data", px, 4 * wn, 2)
        add(_key(EXPAND, d, C=3), "bwd_data", px, 4 * wn, 3, mask_act=LRELU)
        # REDUCE: many -> few channels, lanes per pixel 4 / 8 (constants) and 16 (run time): every OC x ACT; the folds across rows; a mask pass
        for lanes, oc, a in itertools.product((4, 8, 16), (1, 2, 3, 4), (NONE, LRELU, TANH)):
            add(_key(REDUCE, d, C=oc, ACT=a, LC=lanes if lanes < 16 else 0), "fwd", pixels_for(256 // lanes), lanes * wn, oc, act=a, bias=True)
        for lanes in (32, 64):
            add(_key(REDUCE, d, C=2, ACT=TANH), "fwd", pixels_for(256 // lanes), lanes * wn, 2, act=TANH, bias=True)
        add(_key(REDUCE, d, C=2, LC=4), "fwd", pixels_for(64), 4 * wn, 2)
        add(_key(REDUCE, d, C=2, LC=4), "bwd_data", pixels_for(64), 2, 4 * wn)
        add(_key(REDUCE, d, C=3, LC=8), "fwd_mask", pixels_for(32), 8 * wn, 3, mask_act=TANH)
        # EXPAND_PNBWD: the colour layer's data gradient through the norm in front of it: 1, 4 and 64 lanes per pixel
        for groups, ic in ((4, 1), (4, 2), (4, 3), (4, 4), (1, 2), (64, 2)):
            for a, addend in itertools.product((NONE, LRELU), (False, True)):
                add(_key(EXPAND_PNBWD, d, C=ic), "pnbwd", (2, 9, 37), groups * wn, ic, act=a, addend=addend)
        # SINGLE3 / SINGLE: one output channel at 3x3 in the three modes, through both maps that reach each; 96 -> 1 at 1x1 (12 bf16 lanes: no REDUCE)
        for kernel, c in ((SINGLE3, 256), (SINGLE, 64)):
            add(_key(kernel, d), "fwd", (2, 5, 7), c, 1, ks=3, act=LRELU, bias=True)
            add(_key(kernel, d), "bwd_data", (2, 5, 7), 1, c, ks=3)
            add(_key(kernel, d), "fwd", (2, 6, 10), c, 1, ks=3, stride=2)
            add(_key(kernel, d), "bwd_data_t", (2, 3, 5), 1, c, ks=3, stride=2)
            add(_key(kernel, d), "fwd_t", (2, 3, 5), c, 1, ks=3, stride=2)
            add(_key(kernel, d), "bwd_data", (2, 6, 10), 1, c, ks=3, stride=2)
        add(_key(SINGLE, d), "fwd", (2, 5, 7), 96, 1, act=TANH, bias=True)
        # DIRECT: the six OCV x VEC combinations in the three modes on ragged sizes; bias + activation in the kernel, the mask as a pass behind it
        for (ci, co), (ocv, vec) in (((1, 16), (4, 1)), ((8, 2), (2, 4)), ((3, 2), (2, 1)), ((4, 1), (1, 4)), ((3, 3), (1, 1)), ((4, 4), (4, 4))):
            k = _key(DIRECT, d, OCV=ocv, VEC=vec)
            add(k, "fwd", (2, 5, 7), ci, co, ks=3, act=TANH, bias=True)
            add(k, "fwd", (2, 6, 10), ci, co, ks=3, stride=2)
            add(k, "fwd_t", (2, 3, 5), ci, co, ks=3, stride=2)
            add(k, "bwd_data", (2, 5, 7), co, ci, ks=3, mask_act=LRELU)
    return out


CASES = _cases()


def families():
    """(kernel, dtype, mode) of every GPU test, with its cases."""
    out = {}
    for c in CASES:
        out.setdefault((c.key.kernel, c.key.dtype, mode(c)), []).append(c)
    return out


def family_id(f):
    return f"{KERNEL_NAMES[f[0]]}-{DTYPE_NAMES[f[1]]}-{MODE_NAMES[f[2]]}"


def bits_case(c):
    """The cases that also run in their sign-bit form: the bf16 leaky-relu EXPAND results of 32 k channels."""
    return c.key.kernel == EXPAND and c.key.dtype == BF16 and c.call == "fwd" and c.act == LRELU and c.co % 32 == 0


# --------------------------------------------------------------------------------------------------------------------- operands and reference
def out_shape(c):
    if c.call in ("fwd", "fwd_mask"):
        return c.n, c.co, c.h // c.stride, c.w // c.stride
    if c.call == "fwd_t":
        return c.n, c.co, 2 * c.h, 2 * c.w
    return c.n, c.ci, c.h, c.w


def operand_shape(c):
    if c.call in ("fwd", "fwd_t", "fwd_mask"):
        return c.n, c.ci, c.h, c.w
    if c.call == "bwd_data_t":
        return c.n, c.co, 2 * c.h, 2 * c.w
    return c.n, c.co, c.h // c.stride, c.w // c.stride


def inputs(c, seed=5):
    """The operands of a case as stored (CPU; activations rounded to the case's dtype): a dict with a, w, alpha and the optional bias, mask, z, addend."""
    g = torch.Generator().manual_seed(seed)
    dt = TORCH_DTYPE[c.key.dtype]
    a = torch.randn(*operand_shape(c), generator=g)
    contracted = a.shape[1] * c.ks * c.ks
    d = {"a": a.to(dt), "w": torch.randn(c.ks, c.ks, c.ci, c.co, generator=g), "alpha": float((2.0 / contracted) ** 0.5)}
    if c.bias:
        d["bias"] = 0.5 * torch.randn(c.co, generator=g)
    if c.mask_act:
        d["mask"] = torch.randn(*out_shape(c), generator=g).to(dt)
    if c.call == "pnbwd":
        d["z"] = torch.randn(*out_shape(c), generator=g).to(dt)
        if c.addend:
            d["addend"] = torch.randn(*out_shape(c), generator=g).to(dt)
    return d


def conv_map(c, a, w):
    """The map of the case without alpha, in the dtype of its operands: the 3x3 maps by igemm_cover.conv_map, the 1x1 ones as the contraction
    they are."""
    data_grad = c.call in ("bwd_data", "bwd_data_t", "pnbwd")
    if c.ks == 1:
        return torch.einsum("nohw,io->nihw" if data_grad else "nihw,io->nohw", a, w[0, 0])
    call = igemm_cover.Call(c.call, 1 if c.call in ("fwd_t", "bwd_data_t") else 0, c.stride, 1 if data_grad else 0)
    return igemm_cover.conv_map(call, a, w)


def conv64(c, a, w):
    """conv_map in float64."""
    return conv_map(c, a.double(), w.double())


def act64(v, act):
    return torch.tanh(v) if act == TANH else (torch.where(v > 0, v, 0.2 * v) if act == LRELU else v)


def dact64(m, act):
    """act'(.) through the activation's OUTPUT m."""
    m = m.double()
    return 1 - m * m if act == TANH else (torch.where(m > 0, 1.0, 0.2).double() if act == LRELU else torch.ones_like(m))


def finish(c, d, y):
    """What follows the conv (y: alpha times the map, float64): the norm's backward, or bias, activation and mask."""
    if c.call == "pnbwd":   # out = (r (g - z r^2 mean_c(z g)) + addend) * act'(z),  r = rsqrt(mean_c z^2 + eps)
        z = d["z"].double()
        r = torch.rsqrt((z * z).mean(1, keepdim=True) + EPS)
        t = r * (y - z * r * r * (z * y).mean(1, keepdim=True))
        if c.addend:
            t = t + d["addend"].double()
        return t * dact64(z, c.act)
    if c.bias:
        y = y + d["bias"].double().view(1, -1, 1, 1)
    y = act64(y, c.act)
    return y * dact64(d["mask"], c.mask_act) if c.mask_act else y


def reference(c, d):
    return finish(c, d, d["alpha"] * conv64(c, d["a"], d["w"]))


def restated(c, d):
    """An honest kernel: the map in fp32 (torch on the CPU) on the operands as stored, alpha, bias, activation and mask behind it in fp32, one
    store in the case's dtype.  The norm's backward (a composite) is finished in float64."""
    y = d["alpha"] * conv_map(c, d["a"].float(), d["w"].float())
    if c.call == "pnbwd":
        return finish(c, d, y.double()).to(TORCH_DTYPE[c.key.dtype])
    if c.bias:
        y = y + d["bias"].float().view(1, -1, 1, 1)
    y = torch.tanh(y) if c.act == TANH else (torch.where(y > 0, y, 0.2 * y) if c.act == LRELU else y)
    if c.mask_act:
        y = y * dact64(d["mask"], c.mask_act).float()
    return y.to(TORCH_DTYPE[c.key.dtype])


def mag(c, d):
    """cover_bounds' mag: (|alpha| map(|a|, |w|) + |bias|) |act'(mask)| in fp32 on the CPU; None for the norm's backward (a composite: its bound
    is the ceiling alone)."""
    if c.call == "pnbwd":
        return None
    m = abs(d["alpha"]) * conv_map(c, d["a"].float().abs(), d["w"].float().abs())
    if c.bias:
        m = m + d["bias"].float().abs().view(1, -1, 1, 1)
    return m * dact64(d["mask"], c.mask_act).abs().float() if c.mask_act else m


def products(c):
    """K: ks^2 taps of the contracted channels; at most 2 x 2 of them where the transposed walk (T2) reaches an element."""
    return (4 if mode(c) == T2 else c.ks * c.ks) * operand_shape(c)[1]


def extra_roundings(c):
    """e: alpha, the bias add and one fold; a leaky-relu slope or mask factor; 1 - m^2 of a tanh mask."""
    return B.E_BASE + int(c.act == LRELU and c.call != "pnbwd") + (2 if c.mask_act == TANH else int(c.mask_act == LRELU))


def passes_behind(c, r):
    """Whether bias and activation, or the mask, run as a pass of their own behind the kernel (a bf16 result is then rounded twice)."""
    return bool((not r.epilogue_fused and (c.bias or c.act != NONE)) or (c.mask_act and not r.mask_fused))


def roundings(c, r):
    return 0 if c.key.dtype == F32 else (2 if passes_behind(c, r) else 1)


def family(c):
    return KERNEL_NAMES[c.key.kernel]


def bound(c, r, ref, m):
    """The element-wise bound of the case's result under route r (tests/cover_bounds.py)."""
    return B.bound(ref, m, products(c), extra_roundings(c), CEILINGS[family(c)][2], roundings=roundings(c, r),
                   tanh_fwd=c.act == TANH and c.call != "pnbwd")


def macs(c):
    a, o = operand_shape(c), out_shape(c)
    return products(c) * o[0] * o[1] * o[2] * o[3]


def run(K, c, d):
    """The case through its public entry point (gansynth_amd.kernels.HipKernels): the result tensor."""
    def dev(t):
        t = t.to("cuda")
        return t.contiguous(memory_format=torch.channels_last) if t.dim() == 4 else t
    a, w, alpha = dev(d["a"]), dev(d["w"]), d["alpha"]
    bias = dev(d["bias"]) if c.bias else None
    mask = dev(d["mask"]) if c.mask_act else None
    x_shape = (c.n, c.ci, c.h, c.w)
    if c.call == "fwd":
        return K.conv2d_fwd_bias_act(a, w, bias, c.ks, c.stride, alpha, c.act, bits=False)
    if c.call == "fwd_t":
        return K.conv2d_transpose_fwd_bias_act(a, w, bias, alpha, c.act)
    if c.call == "fwd_mask":
        return K.conv2d_fwd_mask(a, w, c.ks, c.stride, alpha, mask, c.mask_act)
    if c.call == "bwd_data":
        return K.conv2d_bwd_data(a, w, x_shape, c.ks, c.stride, alpha, mask=mask, mask_act=c.mask_act)
    if c.call == "bwd_data_t":
        return K.conv2d_transpose_bwd_data(a, w, alpha)
    return K.conv2d_bwd_data_pnbwd(a, w, x_shape, c.ks, c.stride, alpha, dev(d["z"]), EPS, c.act, addend=dev(d["addend"]) if c.addend else None)


def ratio(got, ref):
    return igemm_cover.ratio(got, ref)
