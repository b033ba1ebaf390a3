"""One test case per compiled implicit-GEMM conv kernel -- shared by tests/test_igemm_cover_cpu.py and tests/test_igemm_cover_gpu.py (a plain
helper module: no fixtures, no collection hooks).

The cases are keyed by the table of compiled kernels (gs_conv_igemm_table: conv_igemm.hip's GS_IGEMM_CONFIGS), not by a workload: for every
(mode, dtype, configuration) `find_shapes` searches a fixed grid for the cheapest kernel-role shapes the chooser (gs_conv_igemm_config) routes to
that kernel, `api_call` names the public entry point that reaches the dispatch with such a shape, and `conv_ref64` is the float64 reference the
result is compared with element by element.  A retuned threshold moves the shapes; a kernel nothing reaches any more fails the reachability test.

The plain rows are held element by element to the bound of tests/cover_bounds.py (`plain_bound`): K = 9 ic products (4 ic where the transposed
walk reaches an element with at most 2 x 2 taps), e = 3, an fp32 result inside F_i, a bf16 result (rounded once) inside 2^-8 (|ref_i| + F_i) + F_i.
The bf16 reference takes operand AND weight rounded to bf16: that is how the kernel holds them (its prepared weight is bf16, alpha stays fp32 in
the epilogue).  The fused-norm rows and the sign-bit forms keep the assertions of tests/test_kernels_gpu.py.

Worst max error over max |ref| measured on the MI355X over seeds 0 .. 11 of every plain case of at most 5e7 multiply-adds and seed 0 of the others,
both entry points (1230 comparisons; tests/test_igemm_cover_gpu.py prints the column: IGEMM-COVER-WORST), the suite's ceiling and the ceiling held
here (CEILINGS below; the CPU test holds the two copies together):
    family            measured    suite   here
    plain-f32         7.0e-07     0.001   0.0001
(16 x 6.9e-7 = 1.1e-5 is just over 1e-5: the rule gives 1e-4, not the 1e-5 its neighbours get.)  Beside it: the bf16 rows' worst ratio 3.9e-3 (the
store's own rounding); worst err / bound 0.10 over the fp32 rows and 0.993 over the bf16 rows (a round-to-nearest store alone reaches 1 - 2^-8).

U_BF16_MFMA = 2^-24.  The guide documents the f32 MFMA as a k-ordered fmaf chain and says nothing of how v_mfma_f32_32x32x16_bf16 rounds its
internal adds, so the bf16 rows and the bf16 weight-gradient families ran with u = 2^-24 and the worst err / bound per kernel family was read off:
every element of every bf16-MFMA result is inside.  The bf16 rows here say little (0.993 is the store); the weight gradients of
tests/wgrad_cover.py are fp32 results of the same instruction and sit at 0.23 (conv_wgrad_bf16_kernel), 0.06 (thin_dma), 0.22 (2x2) and 0.07 (2x2_sk)
of their bound, against 0.40 for their fp32 sibling conv_wgrad_kernel at shapes of the same size.  Nothing is outside by any factor: no 2^-23.
"""
import ctypes
import json
import os
import subprocess
import sys
from collections import namedtuple

import torch
import torch.nn.functional as TF

from tests import cover_bounds as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S1, S2, T2 = 0, 1, 2
PLAIN, NORM_FWD, NORM_BWD, NORM_BWD2 = 0, 1, 2, 3
F32, BF16 = 0, 1   # GS_F32, GS_BF16 of include/gansynth_hip.h (tests/test_igemm_cover_cpu.py holds them to gansynth_amd._lib)
MODE_NAMES, DTYPE_NAMES, NORM_NAMES = ("S1", "S2", "T2"), ("f32", "bf16"), ("plain", "normfwd", "normbwd", "normbwd2")
CFG_FIELDS = ("A", "B", "TW", "TG", "RESIDENT", "D", "NORM", "RB", "SPEC")
KNOBS = ("GS_NO_SMALL_TILES", "GS_NO_RB128", "GS_SPEC")
# the chooser's measurement knobs, one setting per child process (they are read once); a kernel belongs to the first setting that reaches it
KNOB_SETTINGS = ({}, {"GS_SPEC": "0"}, {"GS_NO_RB128": "1"}, {"GS_NO_SMALL_TILES": "1"})
MAX_MACS = 2e9   # no chosen case may cost the float64 reference more
# max error over max |ref| a kernel's result may have against conv_ref64.  bf16: the bound of the suite's bf16 conv tests (a result rounded to 8
# mantissa bits is within 2^-9 of its own size).  fp32: the suite's 1e-3 (BASELINE.json north star) is a ceiling.
TOLERANCE = {F32: 1e-3, BF16: 1e-2}
# family -> (worst fp32 ratio measured on the MI355X, the suite's ceiling, the ceiling held here: cover_bounds.ceiling_rule): the docstring's table
CEILINGS = {
    "plain-f32":         (7.0e-07, 0.001, 0.0001),
}

# the search grid of find_shapes (kernel-role shapes)
GRID_N = (1, 2, 4, 8, 16, 32, 64)
GRID_HB = (2, 3, 4, 5, 8, 12, 16, 32)
GRID_WB = (16, 24, 32, 40, 64, 72, 128)
GRID_IC = (16, 32, 64, 96, 128)   # 16: fp32 only (one 64-byte chunk)
GRID_OC = (32, 64, 96, 128, 256, 352, 512)   # 352: see the module docstring of tests/test_igemm_cover_cpu.py (the two T2 A = 1, TG = 3 rows)

Kernel = namedtuple("Kernel", "mode dtype cfg")          # cfg: the nine IgemmCfg fields as a tuple of ints
Shape = namedtuple("Shape", "n hb wb ic oc want")        # kernel-role shape: hb x wb the base grid, ic -> oc what the kernel contracts / produces
# a HipKernels method (`name`) and how it sees a kernel-role shape: `transposed` the transposed-conv family, `stride` the layer's, `data_grad` a data
# gradient (the kernel contracts the layer's OUTPUT channels)
Call = namedtuple("Call", "name transposed stride data_grad")


def kernel_id(k):
    return "-".join([MODE_NAMES[k.mode], DTYPE_NAMES[k.dtype]] + [f"{f}{v}" for f, v in zip(CFG_FIELDS, k.cfg)])


def rows(lib):
    """The table as the library spells it: [mode, bf16_only, A, B, TW, TG, RESIDENT, D, NORM, RB, SPEC] per row."""
    out, got, i = (ctypes.c_int * 11)(), [], 0
    while lib.gs_conv_igemm_table(i, out) == 0:
        got.append(list(out))
        i += 1
    return got


def table(lib):
    """Every compiled (mode, dtype, configuration): a row for bf16, and for fp32 unless it is a bf16-only one."""
    return [Kernel(r[0], dtype, tuple(r[2:])) for r in rows(lib) for dtype in (F32, BF16) if dtype == BF16 or not r[1]]


def config(lib, mode, dtype, s):
    """What the chooser answers for a kernel-role shape under this process's knobs: (configuration, compiled)."""
    out = (ctypes.c_int * 10)()
    rc = lib.gs_conv_igemm_config(mode, s.n, s.hb, s.wb, s.ic, s.oc, dtype, s.want, out)
    assert rc == 0, (rc, lib.gs_last_error())
    return tuple(out[:9]), out[9]


def macs(mode, s):
    """Multiply-adds of the float64 reference for the shape."""
    return 9 * s.ic * s.oc * s.n * s.hb * s.wb * (4 if mode == T2 else 1)


def raggedness(k, s):
    """How many of the two spatial extents leave a partial tile: the width no multiple of TW, the height neither of the tile's (128 B pixels / TW)
    nor of the 4 B rows the chooser counts blocks with."""
    b, tw = k.cfg[1], k.cfg[2]
    return int(s.hb % (128 * b // tw) != 0 and s.hb % (4 * b) != 0) + int(s.wb % tw != 0)


def find_shapes(lib):
    """{kernel: [shape, ...]}: for every kernel the grid reaches under the knobs of THIS process, the cheapest shape and the cheapest ragged one
    (neither extent a multiple of the tile; failing that, one of them).  One entry where the two coincide."""
    best = {}   # kernel -> [cheapest, cheapest with one ragged extent, with both]: (cost, shape)
    out = (ctypes.c_int * 10)()
    for mode in (S1, S2, T2):
        for dtype in (F32, BF16):
            for want in (PLAIN, NORM_FWD, NORM_BWD, NORM_BWD2):
                if api_call(mode, want) is None:
                    continue
                for ic in GRID_IC:
                    if ic == 16 and dtype != F32:
                        continue
                    for oc in GRID_OC:
                        for n in GRID_N:
                            for hb in GRID_HB:
                                for wb in GRID_WB:
                                    rc = lib.gs_conv_igemm_config(mode, n, hb, wb, ic, oc, dtype, want, out)
                                    assert rc == 0, (rc, lib.gs_last_error())
                                    if out[6] != want or out[9] != 1:   # (the fused form was asked for and is not what runs: the plain row's case)
                                        continue
                                    k, s = Kernel(mode, dtype, tuple(out[:9])), Shape(n, hb, wb, ic, oc, want)
                                    slot = best.setdefault(k, [None, None, None])
                                    cand = (macs(mode, s), s)
                                    for level in range(raggedness(k, s) + 1):
                                        if slot[level] is None or cand < slot[level]:
                                            slot[level] = cand
    found = {}
    for k, (any_, one, both) in best.items():
        ragged = both or one
        found[k] = [any_[1]] + ([ragged[1]] if ragged and ragged[1] != any_[1] else [])
    return found


def find_shapes_under(knobs):
    """find_shapes in a fresh interpreter with the chooser's knobs set to `knobs` and nothing else (they are read once per process)."""
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env={**env, **knobs}, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return {Kernel(m, d, tuple(c)): [Shape(*s) for s in shapes] for (m, d, c), shapes in json.loads(r.stdout.strip().splitlines()[-1])}


def assignment():
    """[(knobs, {kernel: shapes})] over KNOB_SETTINGS: every kernel with the first setting that reaches it, the default knobs first."""
    seen, out = set(), []
    for knobs in KNOB_SETTINGS:
        found = find_shapes_under(knobs)
        out.append((knobs, {k: v for k, v in found.items() if k not in seen}))
        seen |= set(found)
    return out


_CALLS = {
    # a plain launch is reached through both entry points of its mode: their weight preparation differs
    (S1, PLAIN): (Call("conv2d_fwd", 0, 1, 0), Call("conv2d_bwd_data", 0, 1, 1)),
    (S2, PLAIN): (Call("conv2d_fwd", 0, 2, 0), Call("conv2d_transpose_bwd_data", 1, 2, 1)),
    (T2, PLAIN): (Call("conv2d_transpose_fwd", 1, 2, 0), Call("conv2d_bwd_data", 0, 2, 1)),
    (S1, NORM_FWD): (Call("conv2d_fwd_bias_act_norm", 0, 1, 0),),
    (S2, NORM_FWD): (Call("conv2d_fwd_bias_act_norm", 0, 2, 0),),
    (T2, NORM_FWD): (Call("conv2d_transpose_fwd_bias_act_norm", 1, 2, 0),),
    (S1, NORM_BWD): (Call("conv2d_bwd_data_pnbwd", 0, 1, 1),),
    (S2, NORM_BWD): (Call("conv2d_transpose_bwd_data_pnbwd", 1, 2, 1),),
    # (T2, NORM_BWD): no data gradient runs as the transposed kernel with a norm behind it
    (S1, NORM_BWD2): (Call("conv2d_fwd_pnbwdbwd", 0, 1, 0),),
    (S2, NORM_BWD2): (Call("conv2d_fwd_pnbwdbwd", 0, 2, 0),),
    (T2, NORM_BWD2): (Call("conv2d_transpose_fwd_pnbwdbwd", 1, 2, 0),),
}


def api_call(mode, want, second=False):
    """The public entry point that reaches the dispatch in `mode` asking for epilogue `want`; None where the ABI has none.  `second`: the other
    entry point of a plain launch."""
    calls = _CALLS.get((mode, want))
    if calls is None:
        return None
    return calls[1 if second else 0]


def layer_args(call, n, hb, wb, ic, oc):
    """Kernel-role shape -> the (n, h, w, ci, co) that entry point takes for it: h x w the conv's input side (the transposed family: its small
    side), and a data gradient contracts the layer's output channels."""
    f = 1 if call.transposed else call.stride
    ci, co = (oc, ic) if call.data_grad else (ic, oc)
    return n, hb * f, wb * f, ci, co


def conv_ref64(call, a, w_hwio, alpha, bf16=False, drop=None):
    """The map behind `call` in float64 on the CPU: the stride-1 / stride-2 conv (TF SAME: an even input is padded at the end only), the stride-2
    transposed conv (out[2i+k] += in[i] w[k], cropped at the end to twice the input) or the data gradient of one of them, from the layer's HWIO
    weight [3, 3, ci, co] and alpha.  `a` is the operand the entry point takes (x, resp. gy for a data gradient), NCHW.  bf16: operand and weight
    are rounded to bf16 first (what the kernels hold; they accumulate in fp32).  drop = (tap, chunk): that tap's 32 contracted channels from
    32 * chunk on are zeroed -- a kernel that loses one stage of its K loop."""
    if bf16:
        a, w_hwio = a.bfloat16(), w_hwio.bfloat16()
    a, w = a.double(), w_hwio.double().clone()
    if drop is not None:
        tap, chunk = drop
        lo = 32 * chunk
        if call.data_grad:
            w[tap // 3, tap % 3, :, lo:lo + 32] = 0
        else:
            w[tap // 3, tap % 3, lo:lo + 32, :] = 0
    return alpha * conv_map(call, a, w)


def conv_map(call, a, w):
    """The map of conv_ref64 without alpha, in the dtype of its operands (float64: the reference; fp32: the scale `conv_mag` and the restatement
    of tests/test_igemm_cover_cpu.py)."""
    oihw, iohw = w.permute(3, 2, 0, 1), w.permute(2, 3, 0, 1)
    if not call.transposed and not call.data_grad:
        return TF.conv2d(a, oihw, padding=1) if call.stride == 1 else TF.conv2d(TF.pad(a, (0, 1, 0, 1)), oihw, stride=2)
    if not call.transposed:   # the conv's adjoint: a transposed conv of gy [n, co] with the same [co, ci] kernel
        if call.stride == 1:
            return TF.conv_transpose2d(a, oihw, padding=1)
        return TF.conv_transpose2d(a, oihw, stride=2)[:, :, :2 * a.shape[2], :2 * a.shape[3]]
    if not call.data_grad:
        return TF.conv_transpose2d(a, iohw, stride=2)[:, :, :2 * a.shape[2], :2 * a.shape[3]]
    return TF.conv2d(TF.pad(a, (0, 1, 0, 1)), iohw, stride=2)   # the transposed conv's adjoint: the stride-2 conv of gy [n, co] with [ci, co] read as (out, in)


def stored(t, bf16):
    """An operand as a plain kernel holds it, in fp32."""
    return t.bfloat16().float() if bf16 else t.float()


def conv_mag(call, a, w_hwio, alpha, bf16=False):
    """cover_bounds' mag of a plain case: |alpha| times the same map on the absolute values of the operands as stored, in fp32 on the CPU."""
    return abs(alpha) * conv_map(call, stored(a, bf16).abs(), stored(w_hwio, bf16).abs())


def conv_restated(call, a, w_hwio, alpha, bf16=False):
    """An honest kernel: the map in fp32 (torch's CPU conv) on the operands as stored, alpha behind it, the bf16 rows' result rounded to bf16."""
    y = alpha * conv_map(call, stored(a, bf16), stored(w_hwio, bf16))
    return y.bfloat16() if bf16 else y


def plain_k(mode, s):
    """The most products an element of a plain case sums: 9 taps of the contracted channels; the transposed walk (T2) reaches an element with at
    most 2 x 2 of them."""
    return (4 if mode == T2 else 9) * s.ic


def plain_bound(kernel, s, ref, mag):
    """The element-wise bound of a plain row's result (tests/cover_bounds.py): fp32, or bf16 rounded once; the bf16 rows run the bf16 MFMA."""
    bf16 = kernel.dtype == BF16
    return B.bound(ref, mag, plain_k(kernel.mode, s), B.E_BASE, CEILINGS["plain-f32"][2], roundings=1 if bf16 else 0, u=B.U_BF16_MFMA if bf16 else B.U)


def operand_shape(call, s):
    """NCHW shape of the operand (x, resp. gy) of `call` at kernel-role shape s: the kernel reads ic channels, on the fine grid at stride 2."""
    f = 2 if (call.stride == 2 and call.transposed == call.data_grad) else 1
    return s.n, s.ic, s.hb * f, s.wb * f


def plain_inputs(call, s, seed):
    """(operand, HWIO weight, alpha) of a plain case: standard normal values, the layers' He scale."""
    g = torch.Generator().manual_seed(seed)
    n, h, w, ci, co = layer_args(call, *s[:5])
    a = torch.randn(*operand_shape(call, s), generator=g)
    wt = torch.randn(3, 3, ci, co, generator=g)
    return a, wt, float((2.0 / (9 * ci)) ** 0.5)


def ratio(got, ref):
    """max error over max |ref|: the measure of every conv test of this suite."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (tuple(got.shape), tuple(ref.shape))
    return float((got - ref).abs().max()) / (float(ref.abs().max()) + 1e-300)


if __name__ == "__main__":   # a child of find_shapes_under: the knobs came with the environment
    from gansynth_amd import _lib
    print(json.dumps([[list(k[:2]) + [list(k.cfg)], [list(s) for s in v]] for k, v in find_shapes(_lib.load()).items()]))
