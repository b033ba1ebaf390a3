"""CPU: the cases of tests/test_wgrad_cover_gpu.py exist and mean something (no GPU: the plan queries answer for the MI355X's 256 CUs).

Reachability: the kernel ids gs_conv_wgrad_plan answers over tests/wgrad_cover.py's grid are exactly wgrad_cover.KERNELS -- a new instantiation, or
one nothing reaches any more, fails -- every kernel has a ragged case and every case stays under MAX_MACS for its float64 reference.
ref64 is held to tests/cpu_kernels.py (autograd of the oracle's convs) per route.  Sensitivity: one zeroed gradient pixel moves ref64 and bias64 by
at least ten tolerances at every chosen case and every sweep case, so the GPU test's bound is not vacuous.  Slice counts: the sweep's cases give the
slice counts they name and between them enter every trip and tail of wgrad_reduce_kernel<4>, <16> and wgrad_reduce_batch_kernel (4 and 16 lanes).
Cuts: over the caps of the stream-K sweep the partitions hold every kind of cut of wgrad_cover.SK_CUT_KINDS, in each conv mode."""
import pytest
import torch

from tests import cover_bounds as B
from tests import wgrad_cover as C


@pytest.fixture(scope="module")
def lib():
    from gansynth_amd import _lib
    assert (C.F32, C.BF16) == (_lib.GS_F32, _lib.GS_BF16) and len(C.PLAN_FIELDS) == _lib.WGRAD_PLAN_INTS
    assert (C.DIRECT, C.THIN, C.MFMA_F32, C.MFMA_BF16, C.THIN_DMA, C.TILE64) == (_lib.WGRAD_DIRECT, _lib.WGRAD_THIN, _lib.WGRAD_F32, _lib.WGRAD_BF16,
                                                                                 _lib.WGRAD_THIN_DMA, _lib.WGRAD_TILE64)
    assert C.knobs_unset(), "the cases are searched under the default knobs"
    lib = _lib.load()
    assert lib.gs_wgrad_cu_cap(0) == 0
    return lib


@pytest.fixture(scope="module")
def shapes(lib):
    return C.find_shapes(lib)


def test_every_compiled_kernel_is_reached_by_a_case_under_the_cap(lib, shapes):
    assert len(C.KERNELS) == 28 == len(set(C.KERNELS))   # 22 MFMA instantiations + 2 direct + 4 thin
    missing = [C.kernel_id(k) for k in C.KERNELS if k not in shapes]
    assert not missing, f"compiled, but no shape of the grid runs them under the default knobs: {missing}"
    assert set(shapes) == set(C.KERNELS), [k for k in shapes if k not in C.KERNELS]
    total = cases = 0
    for k, found in shapes.items():
        assert 1 <= len(found) <= (6 if k.family == C.GROUP else 3)
        ragged = 0
        for s in found:
            for route in C.routes(k):
                route = C.route_for(route, s)
                for n in (s.n, sum(C.deferred_counts(s))):
                    p = C.shape_plan(lib, route, s, k.dtype, n=n)
                    want = k if k.family != C.GROUP else k._replace(family=C.TILE64, tw=p["tw"])
                    assert C.plan_kernel(p, k.dtype) == want, (C.kernel_id(k), route, s, n, p)   # every route, and the deferred form's image count
                    assert (p["ick"], p["ock"], p["hb"], p["wb"], p["swapped"]) == (s.ic, s.oc, s.hb, s.wb, route.transposed)
                    assert C.macs(s, n) <= C.MAX_MACS
                    total += C.macs(s, n)
                    cases += 1
            ragged = max(ragged, C.raggedness(k if k.family != C.GROUP else k._replace(family=C.TILE64, tw=32 if s.wb >= 32 else 16), s,
                                              C.shape_plan(lib, C.route_for(C.routes(k)[0], s), s, k.dtype)))
        assert ragged >= 1, (C.kernel_id(k), found)
    print(f"{len(shapes)} kernels, {sum(len(v) for v in shapes.values())} shapes, {cases} (route, image count) cases, {total:.3g} reference multiply-adds")


def test_plan_queries_refuse_and_report_without_gpu(lib):
    import ctypes
    from gansynth_amd import _lib
    out = (ctypes.c_int * _lib.WGRAD_PLAN_INTS)()
    assert lib.gs_conv_wgrad_plan(None, out) == -1 and lib.gs_conv_wgrad_plan(C._conv(1, 7, 8, 32, 32, 3, 2, 0, C.BF16), out) == -1
    assert lib.gs_conv_wgrad_plan(C._conv(1, 8, 8, 32, 32, 3, 1, 0, C.BF16), None) == -1
    # the top-of-pyramid layer: the LDS-DMA kernel, two blocks per CU on 256 CUs, 16 fold lanes; half the slices under a cap of 128 CUs
    top = dict(n=8, h=128, w=1024, ci=32, co=32, ksize=3, stride=1, transposed=0, dtype=C.BF16)
    p = C.layer_plan(lib, **top)
    assert (p["family"], p["tw"], p["ot"], p["nslices"], p["fold"], p["batch"], p["bias"]) == (C.THIN_DMA, 32, 1, 512, 16, 16, 1)
    with C.cu_cap(lib, 128):
        assert C.layer_plan(lib, **top)["nslices"] == 256
    # a job list: two grouped layers of one mode, a thin one, a three-source 1-channel layer split into single-source jobs
    rows = [(C._CONV1, C.Shape(C.S1, 2, 8, 32, 64, 64, 3), (2, 2), True), (C._CONV1, C.Shape(C.S1, 2, 8, 32, 32, 32, 3), (2,), True),
            (C._CONV1, C.Shape(C.S1, 2, 4, 32, 128, 64, 3), (2,), False), (C._CONV1, C.Shape(C.S1, 2, 2, 16, 1, 16, 3), (2, 1, 2), False)]
    arr, ptr, n = C.make_jobs(rows)
    plan = C.jobs_plan(lib, ptr, n)
    assert [g["mode"] for g in plan["groups"]] == [C.S1] and [j["index"] for j in plan["groups"][0]["jobs"]] == [0, 2]
    g = plan["groups"][0]
    assert (g["total_units"], g["total_runs"], g["nblocks"]) == (4 + 2 * 2, 1 + 2, 4) and [j["unit_base"] for j in g["jobs"]] == [0, 4]
    assert [(s["index"], s["source"], s["family"]) for s in plan["single"]] == [(1, -1, C.THIN_DMA), (3, 0, C.DIRECT), (3, 1, C.DIRECT), (3, 2, C.DIRECT)]
    small = (ctypes.c_int * 4)()
    assert lib.gs_conv_wgrad_jobs_plan(ptr, n, small, 4) == -1 and b"ints needed" in lib.gs_last_error()
    assert lib.gs_conv_wgrad_jobs_plan(None, 0, small, 4) == 2 and list(small[:2]) == [0, 0]


@pytest.mark.parametrize("route,mode", [(C._CONV1, C.S1), (C._CONV2, C.S2), (C._CONVT, C.S2)])
def test_reference_agrees_with_the_cpu_emulation(route, mode):
    """ref64 (nine einsums over shifted slices) against tests/cpu_kernels.py (fp32 autograd of the oracle's convs) at one small ragged shape per route."""
    from tests.cpu_kernels import CpuEmuKernels
    E = CpuEmuKernels()
    s = C.Shape(mode, 2, 3, 5, 32, 64, 3)
    x, gy, alpha = C.inputs(route, s, C.F32, seed=1)
    emu = E.conv2d_transpose_bwd_weight(x, gy, alpha) if route.transposed else E.conv2d_bwd_weight(x, gy, 3, route.stride, alpha)
    ref = C.reference(route, s, x, gy, alpha)
    assert ref.dtype == torch.float64 and tuple(ref.shape) == tuple(emu.shape)
    assert C.ratio(emu, ref) <= 1e-5
    if not route.transposed:
        assert C.ratio(E.channel_sum(gy), C.bias64(gy)) <= 1e-5
        x1, gy1, a1 = C.inputs(C._CONV1, C.Shape(C.S1, 2, 3, 5, 2, 32, 1), C.F32, seed=2)   # the 1 x 1 form of the colour layers
        assert C.ratio(E.conv2d_bwd_weight(x1, gy1, 1, 1, a1), C.ref64(x1, gy1, 1, a1, ksize=1)) <= 1e-5


def _sweep_cases():
    for case in C.SLICE_SWEEP + (C.SLICE_TARGET, C.SCALAR_FOLD):
        for n in case.counts:
            yield case, n


def _moved_by_one_pixel(route, s, dtype, n, with_bias):
    """Zero one pixel of the gradient side -- the last column (the partial tile's, where there is one) of the middle image's last row -- and
    return by how much ref64 (and bias64) move, in the tests' own measure."""
    x, gy, alpha = C.inputs(route, s, dtype, seed=5, n=n)
    ref = C.reference(route, s, x, gy, alpha)
    if route.transposed:   # the kernel's gradient side is the layer's x
        x2, gy2 = x.clone(), gy
        x2[n // 2, :, -1, -1] = 0
    else:
        x2, gy2 = x, gy.clone()
        gy2[n // 2, :, -1, -1] = 0
    moved = [C.ratio(C.reference(route, s, x2, gy2, alpha), ref)]
    if with_bias and not route.transposed:
        moved.append(C.ratio(C.bias64(gy2), C.bias64(gy)))
    return min(moved)


def test_one_lost_pixel_is_ten_tolerances_away(lib, shapes):
    checked, least = 0, None
    for k, found in shapes.items():
        for s in found:
            for route in C.routes(k):
                route = C.route_for(route, s)
                for n in {s.n, sum(C.deferred_counts(s))}:
                    m = _moved_by_one_pixel(route, s, k.dtype, n, with_bias=s.ks == 3)
                    assert m >= 10 * C.TOLERANCE, (C.kernel_id(k), route, s, n, m)
                    least = m if least is None else min(least, m)
                    checked += 1
    sweep = {}
    for case, n in _sweep_cases():
        m = _moved_by_one_pixel(case.route, case.shape, case.dtype, n, with_bias=case.bias)
        assert m >= 10 * C.TOLERANCE, (case.name, n, m)
        sweep[case.name] = min(sweep.get(case.name, m), m)
    for mode in (C.S1, C.S2):
        for rows in (C.SK_SMALL[mode], C.SK_LONG[mode]):
            for route, s, ns, bias in rows:
                m = _moved_by_one_pixel(route, s, C.BF16, sum(ns), with_bias=bias)
                assert m >= 10 * C.TOLERANCE, (route, s, ns, m)
                sweep["stream-K"] = min(sweep.get("stream-K", m), m)
    print(f"{checked} kernel cases, least visible lost pixel {least:.3g}; sweeps: { {k: round(v, 4) for k, v in sweep.items()} }")


def test_sweep_gives_the_slice_counts_it_names_and_enters_every_trip(lib):
    hit = {("reduce", 4): set(), ("reduce", 16): set(), ("batch", 4): set(), ("batch", 16): set()}
    for case, n in _sweep_cases():
        p = C.shape_plan(lib, case.route, case.shape, case.dtype, n=n)
        assert C.plan_kernel(p, case.dtype) == case.kernel, (case.name, n, p)
        if case is C.SCALAR_FOLD:
            assert (p["fold"], p["batch"]) == (0, 0) and (9 * case.shape.ic * case.shape.oc) % 4 != 0, p
            continue
        assert p["nslices"] == n == p["ntiles"] // (1 if p["family"] != C.DIRECT else 64), (case.name, n, p)
        assert p["fold"] == (16 if n > 32 else 4) == p["batch"], (case.name, n, p)
        hit[("reduce", p["fold"])] |= C.reduce_trips(p["fold"], n)
        lanes, trips = C.batch_trips(n)
        assert lanes == p["batch"]
        hit[("batch", lanes)] |= trips
    assert hit[("reduce", 4)] == hit[("reduce", 16)] == {"trip8", "trip2", "tail"}, hit
    assert hit[("batch", 4)] == hit[("batch", 16)] == {"trip4", "single"}, hit
    # the restated conditions, at their thresholds: L lanes enter the 8-slice trip from 7 L + 1 slices on, the batch's 4-slice trip from 3 L + 1
    assert "trip8" not in C.reduce_trips(4, 28) and "trip8" in C.reduce_trips(4, 29) and "trip8" not in C.reduce_trips(16, 112) and "trip8" in C.reduce_trips(16, 113)
    assert "trip4" not in C.batch_trips(12)[1] and "trip4" in C.batch_trips(13)[1] and "trip4" not in C.batch_trips(48)[1] and "trip4" in C.batch_trips(49)[1]
    assert "trip2" not in C.reduce_trips(4, 4) and "trip2" in C.reduce_trips(4, 5) and C.reduce_trips(4, 1) == {"tail"}


def sk_plans(lib, mode):
    """[(cap, group plan)] of the stream-K sweep of a conv mode: the small group at every cap from 1 to its uncapped block count, the long-run
    group uncapped."""
    arr, ptr, n = C.make_jobs(C.SK_SMALL[mode])
    free = C.jobs_plan(lib, ptr, n)
    assert len(free["groups"]) == 1 and not free["single"] and free["groups"][0]["mode"] == mode, free
    out = []
    for cap in range(1, free["groups"][0]["nblocks"] + 1):
        with C.cu_cap(lib, cap):
            g = C.jobs_plan(lib, ptr, n)["groups"][0]
        assert g["nblocks"] == cap and g["total_units"] == free["groups"][0]["total_units"]
        out.append((cap, g))
    arr2, ptr2, n2 = C.make_jobs(C.SK_LONG[mode])
    long_ = C.jobs_plan(lib, ptr2, n2)
    assert len(long_["groups"]) == 1 and not long_["single"]
    out.append((0, long_["groups"][0]))
    return out


@pytest.mark.parametrize("mode", [C.S1, C.S2])
def test_stream_k_sweep_cuts_at_every_kind_of_place(lib, mode):
    plans = sk_plans(lib, mode)
    small = plans[0][1]
    assert (small["total_units"], small["total_runs"], small["njobs"]) == (24, 5, 3)
    assert plans[-2][0] == (12 if mode == C.S1 else 6)   # two units per block at stride 1, four at stride 2
    assert plans[-1][1]["nblocks"] >= 13 and plans[-1][1]["total_runs"] == 1
    hit = {}
    for cap, g in plans:
        for kind in C.sk_cuts(g):
            hit.setdefault(kind, []).append(cap)
    assert set(hit) == C.SK_CUT_KINDS, sorted(C.SK_CUT_KINDS - set(hit))
    assert hit["run over 13 blocks or more"] == [0]
    print(f"mode {C.MODE_NAMES[mode]}: caps per kind of cut {hit}")


# ------------------------------------------------------------------------------------------------ the element-wise bound (tests/cover_bounds.py)
def test_table_is_the_constants_and_the_bound_is_never_weaker():
    """The docstring's table is CEILINGS, every ceiling is what the rule gives for its measurement and none is above the 1e-4 every gradient was
    held to before (fp32 results throughout: no bf16 term)."""
    B.check_table(C.__doc__, C.CEILINGS)
    assert set(C.CEILINGS) == set(C.FAMILY_NAMES) | {"bias", "scalar_fold"}
    for family, (measured, suite, here) in C.CEILINGS.items():
        assert suite == C.TOLERANCE and B.never_weaker(C.TOLERANCE, here, 0), family
    assert {C.unit_roundoff(f) for f in C.BF16_MFMA_FAMILIES} == {B.U_BF16_MFMA} and C.unit_roundoff(C.MFMA_F32) == C.unit_roundoff(C.DIRECT) == B.U


def _small_cases(shapes):
    """(kernel, route, shape, image count) of every chosen case and sweep case of at most 5e7 reference multiply-adds."""
    for k, found in shapes.items():
        for s in found:
            for route in C.routes(k):
                for n in sorted({s.n, sum(C.deferred_counts(s))}):
                    if C.macs(s, n) <= B.SMALL_MACS:
                        yield k, C.route_for(route, s), s, n
    for case, n in _sweep_cases():
        if C.macs(case.shape, n) <= B.SMALL_MACS:
            yield case.kernel, case.route, case.shape, n


def _prefilled(ref, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*ref.shape, generator=g) * 0.5 * float(ref.abs().max())).float()


def test_an_honest_kernel_is_inside_the_bound(shapes):
    """The sums restated in fp32 (torch's CPU einsum) stay inside the bound -- fresh, adding into a pre-filled gradient, and the bias gradient --
    at every case of at most 5e7 multiply-adds."""
    worst, n_cases = 0.0, 0
    for k, route, s, n in _small_cases(shapes):
        x, gy, alpha = C.inputs(route, s, k.dtype, seed=5, n=n)
        ref, mag = C.reference(route, s, x, gy, alpha), C.weight_mag(route, s, x, gy, alpha)
        got, fam, K, u = C.restated(route, s, x, gy, alpha), C.FAMILY_NAMES[k.family], C.weight_products(s, n), C.unit_roundoff(k.family)
        base = _prefilled(ref, 6)
        tag = f"{C.kernel_id(k)} {route.name} {tuple(s)} n {n}"
        for m in (B.measure(tag, got, ref, C.bound(fam, ref, mag, K, u), mag),
                  B.measure(tag + " accumulate", base + got, base.double() + ref, C.bound(fam, base.double() + ref, mag + base.abs(), K, u), mag + base.abs()),
                  B.measure(tag + " bias", gy.float().sum((0, 2, 3)), C.bias64(gy), C.bound("bias", C.bias64(gy), C.bias_mag(gy), C.bias_products([gy.shape])),
                            C.bias_mag(gy))):
            assert m.over == 0 and m.compared > 0 and m.worst <= 1, m.message
            worst = max(worst, m.worst)
        n_cases += 1
    print(f"{n_cases} cases, three honest results each, worst err / bound {worst:.3f}")
    assert n_cases >= 50


def test_subtly_wrong_gradients_pass_the_old_assertion_and_fail_the_bound(shapes):
    """Every result here is fp32, so of the covers' mutants only M5 applies (M1 and M3 are about bf16 results) -- and M5 as the other three
    covers run it (elements under 5 % of the largest scaled by 1 + 2^-6: up to 7.8e-4 of max |ref|) is caught by the old 1e-4 at every case: it
    is evaluated and counted here, and nothing of it is in the gap.  The same mutant at a tenth of the threshold (elements under 0.5 % of the
    largest, up to 7.8e-5 of max |ref|) passes the old assertion and must fail the bound at every case."""
    gap = B.Gap(("M5", "M5 under 0.5 %"))
    for k, route, s, n in _small_cases(shapes):
        x, gy, alpha = C.inputs(route, s, k.dtype, seed=5, n=n)
        ref, mag = C.reference(route, s, x, gy, alpha), C.weight_mag(route, s, x, gy, alpha)
        bnd = C.bound(C.FAMILY_NAMES[k.family], ref, mag, C.weight_products(s, n), C.unit_roundoff(k.family))
        tag = f"{C.kernel_id(k)} {route.name} {tuple(s)} n {n}"
        gap.check("M5", tag, B.stored_as(B.scale_small(ref), bf16=False), ref, bnd, C.TOLERANCE)
        gap.check("M5 under 0.5 %", tag, B.stored_as(B.scale_small(ref, below=0.005), bf16=False), ref, bnd, C.TOLERANCE)
    gap.close(need_half=("M5 under 0.5 %",))
    assert gap.kept["M5"] == 0 and gap.evaluated["M5"] >= 50
