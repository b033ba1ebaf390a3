"""GPU: every compiled weight-gradient kernel, every trip of the slice folds and every kind of stream-K cut against the weight gradient by its
definition in float64 (tests/wgrad_cover.py: ref64 / bias64), element by element (below).

Every test first asks the library what it would launch ON THIS DEVICE (gs_conv_wgrad_plan; for deferred calls gs_conv_wgrad_jobs_plan about the very
job list being launched) and asserts the kernel id, slice count or block count it means, so no test passes on a neighbouring kernel or count.
Every case prints `WGRAD-COVER <id> <route> <shape> <form> fold <fold> ratio ...` before it asserts (run with -s).

a. test_kernel_matches_float64: one test per kernel id of wgrad_cover.KERNELS, at its shapes (cheapest, ragged, several channel tiles), through
   every public route, in three forms -- immediate into a fresh tensor, immediate adding into pre-filled gw (and gb where the route has a bias:
   the bf16 MFMA kernels produce it on the side, everything else takes the channel-sum fallback), and deferred with three (x, gy) pairs of
   different image counts adding into one gw, the middle pair left out of the bias.  The layers the 64 x 64-tile kernel takes run their deferred
   form as a stream-K group, not as TILE64: that form is asserted through the jobs plan and counted towards the GROUP kernel of the mode, whose
   test runs only it.  TILE64 with several sources is reachable only under a measurement knob (GS_NO_WGRAD_GROUPS) and is left out.
b. test_slice_count_sweep: three one-pair-per-block kernels (and a transposed store) on one-tile images, so that slices = images, at the counts
   where wgrad_reduce_kernel<4> / <16> and wgrad_reduce_batch_kernel change trips (wgrad_cover.SWEEP_N), immediate and deferred; a channel-slice
   target through the batched fold; the scalar fold.
c. test_stream_k_cut_sweep: one small group per conv mode at every gs_wgrad_cu_cap from 1 to its uncapped block count, and a long run spread over
   14 blocks (the four-in-flight trip of wgrad_sk_reduce_kernel), every gradient against the reference.

Every element of every gradient is held to the bound of tests/cover_bounds.py (wgrad_cover.bound: min of (K + 3) u of the element's own magnitude
and the family's ceiling), at seeds 0 .. 11 of every case of at most 5e7 multiply-adds and seed 0 of the others -- no longer to 1e-4 of max |ref|,
which no ceiling is above.  The worst ratios measured on the MI355X over the 6781 comparisons of this file are in wgrad_cover's docstring; the
`worst` fixture prints that column when the module is done (WGRAD-COVER-WORST).
"""
import pytest
import torch

from tests import cover_bounds as B
from tests import wgrad_cover as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def K():
    from gansynth_amd import kernels
    assert C.knobs_unset(), "the cases are searched and run under the default knobs"
    k = kernels.HipKernels()
    assert k.lib.gs_wgrad_cu_cap(0) == 0
    return k


@pytest.fixture(scope="module")
def shapes(K):
    return C.find_shapes(K.lib)


def _dev(t, dtype=C.F32):
    t = t.to("cuda", C.TORCH_DTYPE[dtype])
    return t.contiguous(memory_format=torch.channels_last) if t.dim() == 4 else t


def _call(K, route, s, x, gy, alpha, out=None, bias_out=None):
    if route.transposed:
        return K.conv2d_transpose_bwd_weight(x, gy, alpha, out=out)
    return K.conv2d_bwd_weight(x, gy, s.ks, route.stride, alpha, out=out, bias_out=bias_out)


def _fold_name(p, deferred):
    if p["fold"] == 0:
        return "scalar"
    return f"batch{p['batch']}" if deferred else f"reduce{p['fold']}"


@pytest.fixture(scope="module")
def worst():
    """The measurement behind the table of wgrad_cover's docstring: printed when the module is done, over whatever ran.  It checks nothing."""
    w = B.Worst()
    yield w
    w.report("WGRAD-COVER", C.CEILINGS)


def _check(worst, family, tag, got, ref, mag, K, u=B.U):
    """Every element of a gradient inside min(K bound, the family's ceiling) (wgrad_cover.bound)."""
    return B.hold("WGRAD-COVER", tag, got, ref, C.bound(family, ref, mag, K, u), mag, worst, family).ratio


def _family(kernel, plans):
    """The ceiling family of a weight gradient: its kernel's, or the scalar fold's where a plan folds with it."""
    return "scalar_fold" if any(p["fold"] == 0 for p in plans) else C.FAMILY_NAMES[kernel.family]


def _prefill(ref, seed):
    """A pre-filled gradient of the reference's own size, so that what is added stays visible in the sum."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*ref.shape, generator=g) * 0.5 * float(ref.abs().max())).float()


def _run_deferred(K, record):
    """defer, record(), flush -- with the plan of every job list the flush launches."""
    K.defer_wgrad_reductions()
    try:
        record()
        with C.captured_plans(K) as plans:
            K.flush_wgrad_reductions()
    finally:
        K.drop_deferred()   # (nothing is pending after a flush; after a failed one nothing may stay behind for the next test)
    torch.cuda.synchronize()
    return plans


@pytest.mark.parametrize("kernel", C.KERNELS, ids=C.kernel_id)
def test_kernel_matches_float64(K, shapes, worst, kernel):
    assert kernel in shapes, f"{C.kernel_id(kernel)}: no shape of the grid reaches it on this device"
    for s in shapes[kernel]:
        for route in C.routes(kernel):
            for seed in B.seeds_for(C.macs(s, sum(C.deferred_counts(s)))):
                _kernel_case(K, worst, kernel, s, C.route_for(route, s), seed)


def _kernel_case(K, worst, kernel, s, route, seed):
    dt, kid, off, u = kernel.dtype, C.kernel_id(kernel), B.SEED_STRIDE * seed, C.unit_roundoff(kernel.family)
    has_bias = not route.transposed
    p = C.shape_plan(K.lib, route, s, dt)
    if kernel.family != C.GROUP:
        assert C.plan_kernel(p, dt) == kernel, (kid, route, s, p)
        x, gy, alpha = C.inputs(route, s, dt, seed=11 + off)
        ref, refb = C.reference(route, s, x, gy, alpha), C.bias64(gy)
        mag, magb, fam = C.weight_mag(route, s, x, gy, alpha), C.bias_mag(gy), _family(kernel, [p])
        kw, kb = C.weight_products(s, s.n), C.bias_products([gy.shape])
        tag = f"{kid} {route.name} {tuple(s)} seed {seed}"
        _check(worst, fam, f"{tag} fresh fold {_fold_name(p, False)}", _call(K, route, s, _dev(x, dt), _dev(gy, dt), alpha), ref, mag, kw, u)
        base, baseb = _prefill(ref, 12), _prefill(refb, 13)
        gw, gb = _dev(base).contiguous(), (_dev(baseb) if has_bias else None)
        _call(K, route, s, _dev(x, dt), _dev(gy, dt), alpha, out=gw, bias_out=gb)
        _check(worst, fam, f"{tag} accumulate fold {_fold_name(p, False)}", gw, base.double() + ref, mag + base.abs(), kw, u)
        if has_bias:
            _check(worst, "bias", f"{tag} accumulate-bias fold {'rides' if p['bias'] else 'channel-sum'}", gb, baseb.double() + refb, magb + baseb.abs(), kb,
                   u if p["bias"] else B.U)
        if kernel.family == C.TILE64:
            return   # its deferred form is the stream-K group: the GROUP kernel's test
    counts = C.deferred_counts(s)
    pairs = [C.inputs(route, s, dt, seed=20 + i + off, n=n) for i, n in enumerate(counts)]
    alpha = pairs[0][2]
    ref = sum(C.reference(route, s, x, gy, alpha) for x, gy, _ in pairs)
    mag = sum(C.weight_mag(route, s, x, gy, alpha) for x, gy, _ in pairs)
    refb, magb = C.bias64(pairs[0][1]) + C.bias64(pairs[2][1]), C.bias_mag(pairs[0][1]) + C.bias_mag(pairs[2][1])
    kw, kb = C.weight_products(s, sum(counts)), C.bias_products([pairs[0][1].shape, pairs[2][1].shape])
    base, baseb = _prefill(ref, 14), _prefill(refb, 15)
    gw, gb = _dev(base).contiguous(), (_dev(baseb) if has_bias else None)
    held = [(_dev(x, dt), _dev(gy, dt)) for x, gy, _ in pairs]

    def record():
        for i, (x, gy) in enumerate(held):
            _call(K, route, s, x, gy, alpha, out=gw, bias_out=gb if (has_bias and i != 1) else None)
    plans = _run_deferred(K, record)
    assert len(plans) == 1, plans
    rides = False
    if kernel.family == C.GROUP:
        assert not plans[0]["single"] and len(plans[0]["groups"]) == 1, plans
        g = plans[0]["groups"][0]
        assert (g["mode"], g["njobs"], g["total_runs"]) == (kernel.mode, 1, (s.ic // 64) * (s.oc // 64)), g
        fold, fam, rides = "sk", C.FAMILY_NAMES[C.GROUP], True
    else:
        assert not plans[0]["groups"] and plans[0]["single"], plans
        assert all(C.plan_kernel(sp, dt) == kernel for sp in plans[0]["single"]), (kid, plans)
        fold = "+".join(sorted({_fold_name(sp, True) for sp in plans[0]["single"]}))
        fam, rides = _family(kernel, plans[0]["single"]), any(sp["bias"] for sp in plans[0]["single"])
    tag = f"{kid} {route.name} {tuple(s)} seed {seed} deferred{counts}"
    _check(worst, fam, f"{tag} fold {fold}", gw, base.double() + ref, mag + base.abs(), kw, u)
    if has_bias:
        _check(worst, "bias", f"{tag} bias fold {fold}", gb, baseb.double() + refb, magb + baseb.abs(), kb, u if rides else B.U)


@pytest.mark.parametrize("case", C.SLICE_SWEEP + (C.SLICE_TARGET, C.SCALAR_FOLD), ids=lambda c: c.name)
def test_slice_count_sweep(K, worst, case):
    for n in case.counts:
        for seed in B.seeds_for(C.macs(case.shape, n)):
            _slice_case(K, worst, case, n, seed)


def _slice_case(K, worst, case, n, seed):
    dt, s, route, u = case.dtype, case.shape, case.route, C.unit_roundoff(case.kernel.family)
    p = C.shape_plan(K.lib, route, s, dt, n=n)
    assert C.plan_kernel(p, dt) == case.kernel, (case.name, n, p)
    scalar = case is C.SCALAR_FOLD
    assert (p["fold"] == 0) if scalar else (p["nslices"] == n and p["fold"] == (16 if n > 32 else 4) == p["batch"]), (case.name, n, p)
    x, gy, alpha = C.inputs(route, s, dt, seed=31 + n + B.SEED_STRIDE * seed, n=n)
    ref, refb = C.reference(route, s, x, gy, alpha), C.bias64(gy)
    mag, magb, fam = C.weight_mag(route, s, x, gy, alpha), C.bias_mag(gy), _family(case.kernel, [p])
    kw, kb = C.weight_products(s, n), C.bias_products([gy.shape])
    xd, gyd = _dev(x, dt), _dev(gy, dt)
    tag = f"{C.kernel_id(case.kernel)} {route.name} {tuple(s._replace(n=n))} {case.name} seed {seed}"
    if case is C.SLICE_TARGET:
        parent_base = _prefill(torch.ones(3, 3, 5, s.oc) * float(ref.abs().max()), 32)   # a 5-input-channel variable; the layer is its last row
        parent, parent_ref, parent_mag = _dev(parent_base).contiguous(), parent_base.double(), parent_base.abs()
        parent_ref[:, :, 4:5, :] += ref
        parent_mag[:, :, 4:5, :] += mag
        K.defer_wgrad_reductions()
        assert K.wgrad_slice_target_ok(xd, s.oc, 3, 1)
        K.drop_deferred()
        plans = _run_deferred(K, lambda: _call(K, route, s, xd, gyd, alpha, out=parent[:, :, 4:5, :]))
        sp = plans[0]["single"]
        assert len(plans) == 1 and not plans[0]["groups"] and len(sp) == 1 and sp[0]["nslices"] == n and sp[0]["batch"] == (16 if n > 32 else 4), plans
        _check(worst, fam, f"{tag} deferred fold batch{sp[0]['batch']}", parent, parent_ref, parent_mag, kw, u)
        return
    base, baseb = _prefill(ref, 33), _prefill(refb, 34)
    # immediate: wgrad_reduce_kernel<4> / <16> (or the scalar fold)
    gw, gb = _dev(base).contiguous(), (_dev(baseb) if case.bias else None)
    _call(K, route, s, xd, gyd, alpha, out=gw, bias_out=gb)
    _check(worst, fam, f"{tag} accumulate fold {_fold_name(p, False)}", gw, base.double() + ref, mag + base.abs(), kw, u)
    if case.bias:
        _check(worst, "bias", f"{tag} accumulate-bias fold {_fold_name(p, False)}", gb, baseb.double() + refb, magb + baseb.abs(), kb, u)
    if scalar:
        _check(worst, fam, f"{tag} fresh fold scalar", _call(K, route, s, xd, gyd, alpha), ref, mag, kw, u)
    # deferred: wgrad_reduce_batch_kernel, lanes by the entry's slice count (the scalar fold cannot stay pending: folded at once inside the job)
    gw, gb = _dev(base).contiguous(), (_dev(baseb) if case.bias else None)
    plans = _run_deferred(K, lambda: _call(K, route, s, xd, gyd, alpha, out=gw, bias_out=gb))
    sp = plans[0]["single"]
    assert len(plans) == 1 and not plans[0]["groups"] and len(sp) == 1 and C.plan_kernel(sp[0], dt) == case.kernel, plans
    assert (sp[0]["batch"] == 0) if scalar else (sp[0]["nslices"] == n and sp[0]["batch"] == (16 if n > 32 else 4)), sp
    _check(worst, fam, f"{tag} deferred fold {_fold_name(sp[0], True)}", gw, base.double() + ref, mag + base.abs(), kw, u)
    if case.bias:
        _check(worst, "bias", f"{tag} deferred-bias fold {_fold_name(sp[0], True)}", gb, baseb.double() + refb, magb + baseb.abs(), kb, u)


def _group_work(rows, seed):
    """Device operands, float64 references and mags of a stream-K group's layers, computed once:
    [(route, shape, [(x, gy, with bias)], alpha, ref, refb, mag, magb, K of the weights, K of the bias)]."""
    work = []
    for li, (route, s, ns, bias) in enumerate(rows):
        pairs = [C.inputs(route, s, C.BF16, seed=seed + 10 * li + i, n=n) for i, n in enumerate(ns)]
        alpha = pairs[0][2]
        ref = sum(C.reference(route, s, x, gy, alpha) for x, gy, _ in pairs)
        mag = sum(C.weight_mag(route, s, x, gy, alpha) for x, gy, _ in pairs)
        counted = [gy for i, (x, gy, _) in enumerate(pairs) if i != 1] if bias else []
        refb = sum(C.bias64(gy) for gy in counted) if bias else None
        magb = sum(C.bias_mag(gy) for gy in counted) if bias else None
        held = [(_dev(x, C.BF16), _dev(gy, C.BF16), bias and i != 1) for i, (x, gy, _) in enumerate(pairs)]
        work.append((route, s, held, alpha, ref, refb, mag, magb, C.weight_products(s, sum(ns)), C.bias_products([gy.shape for gy in counted])))
    return work


def _group_macs(rows):
    return sum(C.macs(s, sum(ns)) for route, s, ns, bias in rows)


def _run_group(K, worst, work, tag, want_blocks, want_units):
    outs, u = [], C.unit_roundoff(C.GROUP)
    for li, (route, s, held, alpha, ref, refb, mag, magb, kw, kb) in enumerate(work):
        base, baseb = _prefill(ref, 50 + li), (_prefill(refb, 60 + li) if refb is not None else None)
        outs.append((base, baseb, _dev(base).contiguous(), None if baseb is None else _dev(baseb)))

    def record():
        for (route, s, held, alpha, *_), (base, baseb, gw, gb) in zip(work, outs):
            for x, gy, with_b in held:
                _call(K, route, s, x, gy, alpha, out=gw, bias_out=gb if with_b else None)
    plans = _run_deferred(K, record)
    assert len(plans) == 1 and len(plans[0]["groups"]) == 1 and not plans[0]["single"], plans
    g = plans[0]["groups"][0]
    assert (g["nblocks"], g["total_units"], g["njobs"]) == (want_blocks, want_units, len(work)), (tag, g)
    for li, ((route, s, held, alpha, ref, refb, mag, magb, kw, kb), (base, baseb, gw, gb)) in enumerate(zip(work, outs)):
        _check(worst, "group", f"group-{C.MODE_NAMES[s.mode]} {route.name} {tuple(s)} {tag} layer {li} fold sk", gw, base.double() + ref, mag + base.abs(), kw, u)
        if refb is not None:
            _check(worst, "bias", f"group-{C.MODE_NAMES[s.mode]} {route.name} {tuple(s)} {tag} layer {li} bias fold sk", gb, baseb.double() + refb,
                   magb + baseb.abs(), kb, u)
    return g


@pytest.mark.parametrize("mode", [C.S1, C.S2], ids=C.MODE_NAMES)
def test_stream_k_cut_sweep(K, worst, mode):
    free = 12 if mode == C.S1 else 6   # 24 units at two (stride 2: four) per block: tests/test_wgrad_cover_cpu.py holds the cuts these caps give
    seen = set()
    for seed in B.seeds_for(_group_macs(C.SK_SMALL[mode])):
        small = _group_work(C.SK_SMALL[mode], 100 + B.SEED_STRIDE * seed)
        for cap in range(1, free + 1):
            with C.cu_cap(K.lib, cap):
                seen |= C.sk_cuts(_run_group(K, worst, small, f"cap {cap} seed {seed}", cap, 24))
    for seed in B.seeds_for(_group_macs(C.SK_LONG[mode])):
        long_ = _group_work(C.SK_LONG[mode], 300 + B.SEED_STRIDE * seed)
        g = _run_group(K, worst, long_, f"uncapped long run seed {seed}", 14, 28 if mode == C.S1 else 56)
        seen |= C.sk_cuts(g)
    assert seen == C.SK_CUT_KINDS, sorted(C.SK_CUT_KINDS - seen)
    assert K.lib.gs_wgrad_cu_cap(0) == 0
