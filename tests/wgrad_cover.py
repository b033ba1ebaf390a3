"""One test case per compiled weight-gradient kernel, per trip of the slice folds and per kind of stream-K cut -- shared by
tests/test_wgrad_cover_cpu.py and tests/test_wgrad_cover_gpu.py (a plain helper module: no fixtures, no collection hooks).

The cases are keyed by what the library says it would launch (gs_conv_wgrad_plan / gs_conv_wgrad_jobs_plan: the plan the launchers themselves read),
not by a workload: `find_shapes` searches a fixed grid for the cheapest kernel-role shapes the selection routes to each kernel of `KERNELS`,
`routes` names the public calls that reach it, `ref64` is the weight gradient by its definition in float64.  SLICE_SWEEP and the SK_* groups pin the
slice counts and stream-K block counts at which the folds take each of their unrolled trips and tails and the blocks cut the unit list at each kind
of place; tests/test_wgrad_cover_cpu.py proves that from the plans, tests/test_wgrad_cover_gpu.py runs them.

Every gradient is held element by element to the bound of tests/cover_bounds.py (`bound`): K = n Hb Wb (all images of all pairs; a bias gradient:
the pixels of every gy that counts), e = 3, mag with |what the gradient accumulates into|, min of the K bound and the family's ceiling.  All results
are fp32.  The kernels that run v_mfma_f32_32x32x16_bf16 take cover_bounds.U_BF16_MFMA (tests/igemm_cover.py's docstring: 2^-24, with these
families' figures as the evidence).

Worst max error over max |ref| measured on the MI355X over seeds 0 .. 11 of every case of at most 5e7 multiply-adds and seed 0 of the others
(6781 comparisons; tests/test_wgrad_cover_gpu.py prints the column: WGRAD-COVER-WORST), the suite's ceiling and the ceiling held here (CEILINGS
below; the CPU test holds the two copies together):
    family            measured    suite   here
    direct            1.6e-07     0.0001  1e-05
    thin              2.1e-07     0.0001  1e-05
    f32               2.7e-07     0.0001  1e-05
    bf16              2.6e-07     0.0001  1e-05
    thindma           2.5e-07     0.0001  1e-05
    tile64            2.2e-07     0.0001  1e-05
    group             1.5e-07     0.0001  1e-05
    bias              3.2e-06     0.0001  0.0001
    scalar_fold       1.2e-06     0.0001  0.0001
Beside it, worst err / bound per family: direct 0.24, thin 0.26, f32 0.40, bf16 0.23, thindma 0.06, tile64 0.22, group 0.07, bias 0.25,
scalar_fold 0.16.
"""
import contextlib
import ctypes
import os
from collections import namedtuple

import torch

from tests import cover_bounds as B

KNOBS = ("GS_NO_THIN_PAIRS", "GS_NO_THIN_DMA", "GS_NO_WGRAD_GROUPS", "GS_NO_DEFERRED_FOLDS")   # the cases are searched and run with none of them set
S1, S2 = 0, 1
F32, BF16 = 0, 1   # GS_F32, GS_BF16 (tests/test_wgrad_cover_cpu.py holds them, and the families below, to gansynth_amd._lib)
DIRECT, THIN, MFMA_F32, MFMA_BF16, THIN_DMA, TILE64, GROUP = range(7)   # GS_WGRAD_* of include/gansynth_hip.h; GROUP: the stream-K form of TILE64
FAMILY_NAMES = ("direct", "thin", "f32", "bf16", "thindma", "tile64", "group")
MODE_NAMES, DTYPE_NAMES = ("S1", "S2"), ("f32", "bf16")
TORCH_DTYPE = {F32: torch.float32, BF16: torch.bfloat16}
PLAN_FIELDS = ("family", "mode", "tw", "ot", "swapped", "ick", "ock", "hb", "wb", "ntiles", "nslices", "fold", "batch", "bias", "tiles_x", "tiles_y")
MAX_MACS = 5e8      # no case may cost the float64 reference more
TOLERANCE = 1e-4    # max error over max |ref|: the bound of every weight- and bias-gradient test of tests/test_kernels_gpu.py, both dtypes
# family -> (worst ratio measured on the MI355X, the suite's ceiling, the ceiling held here: cover_bounds.ceiling_rule): the docstring's table.
# A kernel family counts with whatever folds its slices; the bias gradients and the scalar fold (wgrad_reduce_scalar_kernel) are families of their own.
CEILINGS = {
    "direct":            (1.6e-07, 0.0001, 1e-05),
    "thin":              (2.1e-07, 0.0001, 1e-05),
    "f32":               (2.7e-07, 0.0001, 1e-05),
    "bf16":              (2.6e-07, 0.0001, 1e-05),
    "thindma":           (2.5e-07, 0.0001, 1e-05),
    "tile64":            (2.2e-07, 0.0001, 1e-05),
    "group":             (1.5e-07, 0.0001, 1e-05),
    "bias":              (3.2e-06, 0.0001, 0.0001),
    "scalar_fold":       (1.2e-06, 0.0001, 0.0001),
}
BF16_MFMA_FAMILIES = (MFMA_BF16, THIN_DMA, TILE64, GROUP)   # the kernels that run v_mfma_f32_32x32x16_bf16: their u is cover_bounds.U_BF16_MFMA

# family, conv mode, pixel-tile width, OT (thin: 1 when x is the wide side), dtype.  The direct kernel takes the conv mode as an argument: one id per dtype.
Kernel = namedtuple("Kernel", "family mode tw ot dtype")
Shape = namedtuple("Shape", "mode n hb wb ic oc ks")   # kernel-role shape: hb x wb the gradient side's grid, ic -> oc what the kernel contracts / produces
Route = namedtuple("Route", "name transposed stride")

KERNELS = (
    [Kernel(MFMA_F32, m, tw, 1, F32) for m in (S1, S2) for tw in (16, 32)]                          # conv_wgrad_kernel<float, MODE, TW>
    + [Kernel(MFMA_BF16, m, tw, ot, BF16) for m in (S1, S2) for tw in (16, 32) for ot in (1, 2)]   # conv_wgrad_bf16_kernel<MODE, TW, OT>
    + [Kernel(THIN_DMA, m, 32, ot, BF16) for m in (S1, S2) for ot in (1, 2)]                       # conv_wgrad_bf16_thin_dma_kernel<MODE, OT>
    + [Kernel(TILE64, m, tw, 2, BF16) for m in (S1, S2) for tw in (16, 32)]                        # conv_wgrad_bf16_2x2_kernel<MODE, TW>
    + [Kernel(GROUP, m, 32, 2, BF16) for m in (S1, S2)]                                            # conv_wgrad_bf16_2x2_sk_kernel<MODE>
    + [Kernel(DIRECT, S1, 0, 0, d) for d in (F32, BF16)]                                           # conv_wgrad_direct_kernel<T>
    + [Kernel(THIN, S1, 0, wide_x, d) for d in (F32, BF16) for wide_x in (0, 1)]                   # thin_wgrad_kernel<T, WIDE_IS_X>
)

GRID_N = (1, 2, 3)
GRID_HB = (1, 2, 3, 5, 8, 9, 17)
GRID_WB = (7, 16, 24, 32, 33, 40, 64, 72)
GRID_C = (32, 64, 96, 128)
GRID_FEW = (1, 2, 3)   # one side of the direct / thin kernels' layers


def kernel_id(k):
    return f"{FAMILY_NAMES[k.family]}-{MODE_NAMES[k.mode]}-TW{k.tw}-OT{k.ot}-{DTYPE_NAMES[k.dtype]}"


def ratio(got, ref):
    """max error over max |ref|: the measure of every conv test of this suite."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (tuple(got.shape), tuple(ref.shape))
    return float((got - ref).abs().max()) / (float(ref.abs().max()) + 1e-300)


# ------------------------------------------------------------------------------------------------------------------ the float64 reference
def ref64(x, gy, stride, alpha, transposed=False, ksize=3, dtype=torch.float64):
    """The weight gradient by its definition, float64, HWIO: ksize^2 einsums nchw,nohw->co over shifted slices of the padded operand -- no conv call,
    no autograd.  stride 1: x padded by ksize // 2 all round; stride 2: x padded at the end only (TF SAME on an even input), slices
    [ky : ky + 2 Hb : 2]; transposed conv: gy padded at the end, gw[ky, kx, ci, co] = sum x[n, ci, i, j] gy[n, co, 2 i + ky, 2 j + kx].
    (dtype: fp32 for the scale `weight_mag` and the restatement of tests/test_wgrad_cover_cpu.py.)"""
    x, gy = x.to(dtype), gy.to(dtype)
    ci, co = x.shape[1], gy.shape[1]
    gw = torch.zeros(ksize, ksize, ci, co, dtype=dtype)
    if transposed:
        assert ksize == 3 and stride == 2 and gy.shape[2:] == (2 * x.shape[2], 2 * x.shape[3])
        a, hb, wb, step = torch.nn.functional.pad(gy, (0, 1, 0, 1)), x.shape[2], x.shape[3], 2
    elif stride == 2:
        assert ksize == 3 and x.shape[2:] == (2 * gy.shape[2], 2 * gy.shape[3])
        a, hb, wb, step = torch.nn.functional.pad(x, (0, 1, 0, 1)), gy.shape[2], gy.shape[3], 2
    else:
        assert stride == 1 and x.shape[2:] == gy.shape[2:]
        p = ksize // 2
        a, hb, wb, step = torch.nn.functional.pad(x, (p, p, p, p)), gy.shape[2], gy.shape[3], 1
    for ky in range(ksize):
        for kx in range(ksize):
            win = a[:, :, ky:ky + step * hb:step, kx:kx + step * wb:step]
            gw[ky, kx] = torch.einsum("nchw,nohw->co", x, win) if transposed else torch.einsum("nchw,nohw->co", win, gy)
    return alpha * gw


def weight_mag(route, s, x, gy, alpha):
    """cover_bounds' mag of a weight gradient (without what it accumulates into): the same sums over |x| |gy|, fp32 on the CPU."""
    return ref64(x.abs(), gy.abs(), route.stride, abs(alpha), transposed=bool(route.transposed), ksize=s.ks, dtype=torch.float32)


def restated(route, s, x, gy, alpha):
    """An honest kernel: the same sums in fp32 (torch on the CPU)."""
    return ref64(x, gy, route.stride, alpha, transposed=bool(route.transposed), ksize=s.ks, dtype=torch.float32)


def bias_mag(gy):
    return gy.float().abs().sum((0, 2, 3))


def weight_products(s, n):
    """K of a weight gradient: every pixel of the gradient side's grid, over all n images."""
    return n * s.hb * s.wb


def bias_products(gy_shapes):
    """K of a bias gradient: every pixel of every gy that counts towards it."""
    return sum(g[0] * g[2] * g[3] for g in gy_shapes)


def unit_roundoff(kernel_family):
    return B.U_BF16_MFMA if kernel_family in BF16_MFMA_FAMILIES else B.U


def bound(family, ref, mag, K, u=B.U):
    """The element-wise bound of a weight or bias gradient (fp32 results; tests/cover_bounds.py): min of the K bound and the family's ceiling."""
    return B.bound(ref, mag, K, B.E_BASE, CEILINGS[family][2], u=u)


def bias64(gy):
    return gy.double().sum((0, 2, 3))


# ------------------------------------------------------------------------------------------------------------------------- the plan queries
def _conv(n, h, w, ci, co, ksize, stride, transposed, dtype):
    from gansynth_amd import _lib
    return _lib.GsConv(n, h, w, ci, co, ksize, stride, transposed, dtype, 0, 1.0, None, 0)


def layer_plan(lib, n, h, w, ci, co, ksize, stride, transposed, dtype):
    """gs_conv_wgrad_plan for a LAYER (its own forward labelling, n images in all) as a dict over PLAN_FIELDS."""
    out = (ctypes.c_int * len(PLAN_FIELDS))()
    rc = lib.gs_conv_wgrad_plan(_conv(n, h, w, ci, co, ksize, stride, transposed, dtype), out)
    assert rc == 0, (rc, lib.gs_last_error())
    return dict(zip(PLAN_FIELDS, out))


def plan_kernel(p, dtype):
    """The kernel id a per-layer plan names."""
    if p["family"] == DIRECT:
        return Kernel(DIRECT, S1, 0, 0, dtype)
    return Kernel(p["family"], p["mode"], p["tw"], p["ot"], dtype)


def routes(kernel):
    """The public calls (gansynth_amd.kernels.HipKernels) that reach the kernel: conv2d_bwd_weight at the stride of its mode; every stride-2
    instantiation also through conv2d_transpose_bwd_weight (swapped sides, transposed store)."""
    if kernel.family in (DIRECT, THIN):
        return (Route("conv2d_bwd_weight", 0, 1),)   # (a direct shape of mode S2 runs at stride 2: layer_args)
    if kernel.mode == S1:
        return (Route("conv2d_bwd_weight", 0, 1),)
    return (Route("conv2d_bwd_weight", 0, 2), Route("conv2d_transpose_bwd_weight", 1, 2))


def route_for(route, s):
    """The route at the stride the SHAPE's mode asks for (the direct kernel's id spans both modes)."""
    return route if route.transposed else Route(route.name, 0, 2 if s.mode == S2 else 1)


def layer_args(route, s):
    """Kernel-role shape -> (x shape, gy shape, (h, w, ci, co) of the layer) for the route.  The transposed layer's x is its small side with the
    kernel's OUTPUT channels: the kernel contracts gy (2 hb x 2 wb, ic channels) against it."""
    if route.transposed:
        return (s.n, s.oc, s.hb, s.wb), (s.n, s.ic, 2 * s.hb, 2 * s.wb), (s.hb, s.wb, s.oc, s.ic)
    f = route.stride
    return (s.n, s.ic, f * s.hb, f * s.wb), (s.n, s.oc, s.hb, s.wb), (f * s.hb, f * s.wb, s.ic, s.oc)


def shape_plan(lib, route, s, dtype, n=None):
    (_, _, _, _), _, (h, w, ci, co) = layer_args(route, s)
    return layer_plan(lib, s.n if n is None else n, h, w, ci, co, s.ks, route.stride, route.transposed, dtype)


def macs(s, n=None):
    return s.ks * s.ks * s.ic * s.oc * (s.n if n is None else n) * s.hb * s.wb


def tile_dims(k):
    """(TH, TW) of an MFMA kernel's pixel tile."""
    if k.family == MFMA_F32:
        npix = 64 if k.mode == S2 else 128
    elif k.family == MFMA_BF16:
        npix = 128 if k.mode == S2 else 256
    else:
        npix = 64 if k.mode == S2 else 256
    return npix // k.tw, k.tw


def raggedness(k, s, p):
    """How many of the two extents hold more than one tile and leave a partial one (2 only with more than one image, so that the image index
    counts); the direct / thin kernels: a pixel count that fills neither the last slice nor the last round of a block's four (thin:
    256 / (C / 4)) pixel lanes (2 for the direct kernel only at 3 x 3, stride 1: the cheapest shapes are 1 x 1)."""
    if k.family in (DIRECT, THIN):
        npix = s.n * s.hb * s.wb
        lanes = 4 if k.family == DIRECT else 256 // (max(s.ic, s.oc) // 4)
        level = int(npix % p["nslices"] != 0) + int(npix % lanes != 0)
        return min(level, 1) if (k.family == DIRECT and not (s.ks == 3 and s.mode == S1 and s.n > 1)) else level
    th, tw = tile_dims(k)
    level = int(s.hb > th and s.hb % th != 0) + int(s.wb > tw and s.wb % tw != 0)
    return min(level, 1) if s.n < 2 else level


def channel_spread(k, s):
    """2: more than one channel tile on each side and ic != oc (a swapped index shows); 1: more than one block over the channels and ic != oc;
    the direct kernel: a stride-2 shape of more than one 64-element block."""
    if k.family == DIRECT:
        return 2 if (s.mode == S2 and s.ks * s.ks * s.ic * s.oc > 64 and s.ic != s.oc) else 0
    if k.family == THIN or s.ic == s.oc:
        return 0
    ti, to = (64, 64) if k.family == TILE64 else (32, 32 * k.ot)
    a, b = s.ic // ti, s.oc // to
    return 2 if (a > 1 and b > 1) else (1 if a * b > 1 else 0)


def grid_shapes():
    for mode in (S1, S2):
        for ic in GRID_C:
            for oc in GRID_C:
                for n in GRID_N:
                    for hb in GRID_HB:
                        for wb in GRID_WB:
                            yield Shape(mode, n, hb, wb, ic, oc, 3)
    for ks, mode in ((1, S1), (3, S1), (3, S2)):   # the direct and thin kernels' layers: few channels on one side at least
        for ic in GRID_FEW + GRID_C:
            for oc in GRID_FEW + GRID_C:
                if ic in GRID_FEW or oc in GRID_FEW:
                    for n in GRID_N:
                        for hb in GRID_HB:
                            for wb in GRID_WB:
                                yield Shape(mode, n, hb, wb, ic, oc, ks)


def find_shapes(lib):
    """{kernel: [shape, ...]} over the grid under THIS process's knobs: the cheapest shape, the cheapest with a partial tile in both extents (failing
    that in one), the cheapest with more than one channel tile on each side and ic != oc (failing that, more than one block over the channels).
    The GROUP kernels take the shapes of the TILE64 kernels of their mode (the deferred form of those layers)."""
    best = {}
    for s in grid_shapes():
        for dtype in (F32, BF16):
            if macs(s) > MAX_MACS:
                continue
            p = shape_plan(lib, route_for(Route("conv2d_bwd_weight", 0, 1), s), s, dtype)
            k = plan_kernel(p, dtype)
            slot = best.setdefault(k, {})
            cand = (macs(s), s)
            keys = [("any", 0)] + [("ragged", lv) for lv in range(1, raggedness(k, s, p) + 1)] + [("spread", lv) for lv in range(1, channel_spread(k, s) + 1)]
            for key in keys:
                if key not in slot or cand < slot[key]:
                    slot[key] = cand
    found = {}
    for k, slot in best.items():
        picks = [slot[("any", 0)][1]]
        for name in ("ragged", "spread"):
            pick = slot.get((name, 2)) or slot.get((name, 1))
            if pick and pick[1] not in picks:
                picks.append(pick[1])
        found[k] = picks
    for mode in (S1, S2):
        grouped = [s for k, v in found.items() if k.family == TILE64 and k.mode == mode for s in v]
        if grouped:
            found[Kernel(GROUP, mode, 32, 2, BF16)] = grouped
    return found


def inputs(route, s, dtype, seed, n=None):
    """(x, gy, alpha): standard normal, NCHW fp32 -- bf16 cases rounded to bf16 first (kernel and reference see the same values: products are then
    exact in fp32 and only the accumulation order differs)."""
    g = torch.Generator().manual_seed(seed)
    xs, gs, _ = layer_args(route, s if n is None else s._replace(n=n))
    x, gy = torch.randn(*xs, generator=g), torch.randn(*gs, generator=g)
    if dtype == BF16:
        x, gy = x.bfloat16().float(), gy.bfloat16().float()
    return x, gy, float((2.0 / (s.ks * s.ks * xs[1])) ** 0.5)


def reference(route, s, x, gy, alpha):
    return ref64(x, gy, route.stride, alpha, transposed=bool(route.transposed), ksize=s.ks)


def deferred_counts(s):
    """Image counts of the pairs of the deferred multi-source form at a shape: three pairs, different counts."""
    return (s.n, 1, 2) if s.n != 2 else (2, 1, 3)


# ----------------------------------------------------------------------------------------------------------------------- the jobs plan
def jobs_plan(lib, jobs_ptr, njobs):
    """gs_conv_wgrad_jobs_plan parsed: {"groups": [{mode, njobs, total_units, total_runs, nblocks, jobs: [{index, unit_base, run_base, ntiles, nct}]}],
    "single": [{index, source, **per-layer plan}]}."""
    room = 2 + 5 * (1 + njobs) * max(njobs, 1) + 4 * njobs * (2 + len(PLAN_FIELDS))
    out = (ctypes.c_int * room)()
    n = lib.gs_conv_wgrad_jobs_plan(jobs_ptr, njobs, out, room)
    assert n >= 2, (n, lib.gs_last_error())
    v, pos = list(out[:n]), 2
    plan = {"groups": [], "single": []}
    for _ in range(v[0]):
        g = dict(zip(("mode", "njobs", "total_units", "total_runs", "nblocks"), v[pos:pos + 5]), jobs=[])
        pos += 5
        for _ in range(g["njobs"]):
            g["jobs"].append(dict(zip(("index", "unit_base", "run_base", "ntiles", "nct"), v[pos:pos + 5])))
            pos += 5
        plan["groups"].append(g)
    for _ in range(v[1]):
        plan["single"].append(dict(zip(("index", "source") + PLAN_FIELDS, v[pos:pos + 2 + len(PLAN_FIELDS)])))
        pos += 2 + len(PLAN_FIELDS)
    assert pos == n
    return plan


def make_jobs(layers, dtype=BF16):
    """A GsWgradJob array for host-only planning from (route, shape, image counts per pair, with bias) rows: pointers that are never dereferenced,
    a gradient of its own per layer.  -> (array kept alive, pointer, count)."""
    from gansynth_amd import _lib
    arr = (_lib.GsWgradJob * len(layers))()
    for i, (route, s, ns, bias) in enumerate(layers):
        jb = arr[i]
        _, _, (h, w, ci, co) = layer_args(route, s)
        for j, n in enumerate(ns):
            jb.x[j], jb.gy[j], jb.n[j] = 0x100000 * (8 * i + j + 1), 0x100000 * (8 * i + j + 5), n
        jb.nsrc, jb.bias_mask, jb.gw, jb.gb = len(ns), (sum(1 << j for j in range(len(ns)) if j != 1) if bias else 0), 0x1000 * (i + 1), (0x800 * (2 * i + 1) if bias else None)
        jb.h, jb.w, jb.ci, jb.co, jb.ksize, jb.stride, jb.transposed = h, w, ci, co, s.ks, route.stride, route.transposed
        jb.alpha, jb.accumulate, jb.dtype, jb.gw_ci_stride = 0.5, 1, dtype, 0
    return arr, ctypes.cast(arr, ctypes.c_void_p), len(layers)


@contextlib.contextmanager
def captured_plans(K):
    """Every gs_conv_wgrad_jobs call of `K` inside the block first asks gs_conv_wgrad_jobs_plan about the very job list it launches; the parsed
    plans collect in the list this yields."""
    plans, real = [], K.lib.gs_conv_wgrad_jobs

    def launch(ptr, njobs, ws, ws_bytes, stream):
        plans.append(jobs_plan(K.lib, ptr, njobs))
        return real(ptr, njobs, ws, ws_bytes, stream)
    K.lib.gs_conv_wgrad_jobs = launch
    try:
        yield plans
    finally:
        K.lib.gs_conv_wgrad_jobs = real


@contextlib.contextmanager
def cu_cap(lib, cap):
    """gs_wgrad_cu_cap(cap) around the block; 0 (the whole chip) after it, whatever happens, and the value each call returns is checked."""
    was = lib.gs_wgrad_cu_cap(cap)
    try:
        assert was == 0, was
        yield
    finally:
        back = lib.gs_wgrad_cu_cap(0)
    assert back == cap, (back, cap)


# ---------------------------------------------------------------------------------------------------------- the folds' trips, restated
def reduce_trips(lanes, nslices):
    """wgrad_reduce_kernel<lanes>: which of its loops some slice lane enters -- the 8-slice trip, the 2-slice trip, the single tail."""
    hit = set()
    for sl in range(lanes):
        k = sl
        while k + 7 * lanes < nslices:
            hit.add("trip8")
            k += 8 * lanes
        while k + lanes < nslices:
            hit.add("trip2")
            k += 2 * lanes
        if k < nslices:
            hit.add("tail")
    return hit


def batch_trips(nslices):
    """wgrad_reduce_batch_kernel: lanes by the entry's slice count, the 4-slice trip, the singles."""
    lanes, hit = (16 if nslices > 32 else 4), set()
    for sl in range(lanes):
        k = sl
        while k + 3 * lanes < nslices:
            hit.add("trip4")
            k += 4 * lanes
        while k < nslices:
            hit.add("single")
            k += lanes
    return lanes, hit


def sk_block_of(u, nb, total):
    return ((u + 1) * nb - 1) // total   # conv_shared.h


def sk_cuts(group):
    """The kinds of place at which the blocks of a stream-K group (a jobs-plan group) cut its unit list, and how its runs are owned."""
    total, nb = group["total_units"], group["nblocks"]
    runs = [(j["unit_base"] + ct * j["ntiles"], j["unit_base"] + (ct + 1) * j["ntiles"]) for j in group["jobs"] for ct in range(j["nct"])]
    assert runs and runs[0][0] == 0 and runs[-1][1] == total and all(a[1] == b[0] for a, b in zip(runs, runs[1:])) and len(runs) == group["total_runs"]
    starts, ends = {r[0] for r in runs}, {r[1] for r in runs}
    layer_edges = {j["unit_base"] for j in group["jobs"]} - {0}
    hit = set()
    for b in range(nb):
        u0, u1 = b * total // nb, (b + 1) * total // nb
        if u0 >= u1:
            continue
        if u0 not in starts:
            hit.add("starts mid-run")
        if u1 not in ends:
            hit.add("ends mid-run")
        if u0 not in starts and u1 not in ends and any(u0 < a and e < u1 for a, e in runs):
            hit.add("whole run between two partial ones")
        if any(u0 < e < u1 for e in layer_edges):
            hit.add("crosses a layer boundary")
    for a, e in runs:
        spread = sk_block_of(e - 1, nb, total) - sk_block_of(a, nb, total) + 1
        if spread == 1:
            hit.add("run owned by one block")
        if spread >= 13:
            hit.add("run over 13 blocks or more")   # the four-partials-in-flight trip of wgrad_sk_reduce_kernel: b + 12 <= b1
    return hit


SK_CUT_KINDS = {"starts mid-run", "ends mid-run", "whole run between two partial ones", "crosses a layer boundary", "run owned by one block",
                "run over 13 blocks or more"}

# ---------------------------------------------------------------------------------------------------------------------- the sweeps
# images of exactly one pixel tile (128 pixels), one (ic, oc) pair per block: ntiles = N = nslices for every N below
SWEEP_N = (1, 2, 3, 4, 5, 8, 9, 13, 17, 29, 32, 33, 48, 49, 65, 113, 129)
SliceCase = namedtuple("SliceCase", "name kernel route shape dtype counts bias")   # shape.n is a placeholder: every count of `counts` runs
_CONV1, _CONV2, _CONVT = Route("conv2d_bwd_weight", 0, 1), Route("conv2d_bwd_weight", 0, 2), Route("conv2d_transpose_bwd_weight", 1, 2)
SLICE_SWEEP = (
    SliceCase("f32-32to32", Kernel(MFMA_F32, S1, 32, 1, F32), _CONV1, Shape(S1, 1, 4, 32, 32, 32, 3), F32, SWEEP_N, False),
    SliceCase("bf16-32to32-w16", Kernel(MFMA_BF16, S1, 16, 1, BF16), _CONV1, Shape(S1, 1, 8, 16, 32, 32, 3), BF16, SWEEP_N, True),   # with gb: the slice stride holds the bias row
    SliceCase("bf16-s2-32to32-w16", Kernel(MFMA_BF16, S2, 16, 1, BF16), _CONV2, Shape(S2, 1, 8, 16, 32, 32, 3), BF16, SWEEP_N, False),
    SliceCase("bf16-transposed-store", Kernel(MFMA_BF16, S2, 16, 1, BF16), _CONVT, Shape(S2, 1, 8, 16, 32, 32, 3), BF16, (3, 33, 65), False),
)
# a channel-slice target (out = parent[:, :, lo:hi, :], deferred): the 1-input-channel direct kernel on 8 x 8 images, one slice per image
SLICE_TARGET = SliceCase("direct-channel-slice", Kernel(DIRECT, S1, 0, 0, BF16), _CONV1, Shape(S1, 1, 8, 8, 1, 16, 3), BF16, (13, 49), False)
# an element count that is no multiple of 4: the scalar fold
SCALAR_FOLD = SliceCase("direct-scalar-fold", Kernel(DIRECT, S1, 0, 0, F32), _CONV1, Shape(S1, 3, 5, 7, 3, 3, 3), F32, (3,), False)

# stream-K groups: (route, kernel-role shape, image counts of the pairs, with bias).  A pair list with a middle entry leaves it out of the bias.
SK_SMALL = {
    # (the one-run layer in the middle: at five blocks, block 2 holds that run whole between the tail of one run and the head of another)
    S1: ((_CONV1, Shape(S1, 2, 9, 40, 128, 64, 3), (1, 1), True), (_CONV1, Shape(S1, 2, 8, 32, 64, 64, 3), (2,), True),
         (_CONV1, Shape(S1, 3, 2, 16, 64, 128, 3), (3,), True)),
    S2: ((_CONV2, Shape(S2, 2, 3, 40, 128, 64, 3), (1, 1), True), (_CONV2, Shape(S2, 2, 2, 32, 64, 64, 3), (2,), True),
         (_CONVT, Shape(S2, 3, 2, 16, 64, 128, 3), (3,), False)),
}
SK_LONG = {
    S1: ((_CONV1, Shape(S1, 28, 8, 32, 64, 64, 3), (28,), True),),
    S2: ((_CONV2, Shape(S2, 14, 8, 32, 64, 64, 3), (14,), True),),
}


def knobs_unset():
    return not any(k in os.environ for k in KNOBS)
