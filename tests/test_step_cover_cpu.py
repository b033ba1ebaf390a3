"""CPU: the cases of tests/test_step_cover_gpu.py exist and mean something (tests/step_cover.py).

- References: the float64 Adam against the suite's torch-CPU TF-Adam (tests/cpu_kernels.py), the float64 losses against torch.autograd.grad of the
  loss written from the definition (models.py:39-65 of the reference: mean softplus(-r) + softplus(f) + weight * penalty; mean softplus(-f) +
  weight / (sumsq + eps)), the embedding gradient against autograd of an index-select and the chosen index against torch.argmax, the three prep
  layouts against w.transpose, a tap flip and a copy written element by element.
- Bounds: for every case an fp32 numpy restatement of the kernel's arithmetic, once with and once without the multiply-add fused, stays within the
  case's bound; the margin is printed (run with -s).  numpy's fp32 exp and log1p are within the 3 ulp the loss bounds assume of them.
- Case tables: every edge the GPU file is there for is reached, by counting.
- Refusals: the entry points answer what they refuse before any launch (what tests/test_abi_cpu.py does not already hold)."""
import numpy as np
import pytest
import torch

from tests import step_cover as C


@pytest.fixture(scope="module")
def lib():
    from gansynth_amd import _lib
    assert (_lib.GS_F32, _lib.GS_BF16) == (C.F32, C.BF16)
    assert (_lib.PREP_CONV_FWD, _lib.PREP_CONV_BWD_DATA, _lib.PREP_CONVT_FWD, _lib.PREP_CONVT_BWD_DATA) == (C.PREP_FWD, C.PREP_BWD_DATA, C.PREP_T_FWD, C.PREP_T_BWD_DATA)
    return _lib.load()


def _margin(tag, name, got, ref, bound):
    err = np.abs(C.value64(got) - ref)
    worst = float(np.max(np.where(err == 0, 0.0, err / np.maximum(bound, 1e-300))))
    print(f"STEP-COVER-CPU {tag} {name} restatement / bound {worst:.3f}")
    return worst


# ------------------------------------------------------------------------------------------------------------------------------ Adam
def test_adam_reference_is_tf_adam():
    from tests.cpu_kernels import CpuEmuKernels
    E = CpuEmuKernels()
    for c in C.ADAM_CASES:
        if c.n not in (7, 257, 1026):
            continue
        d = C.adam_inputs(c)
        s = slice(192, None) if c.n >= 255 else slice(None)   # (the plain draws: an fp32 reference says nothing about the cancelling and the huge ones)
        p, g, m, v = (torch.from_numpy(d[k][s].astype(np.float64)) for k in "pgmv")
        E.adam_tf_step(p, g, m, v, float(C.ADAM_LR_T), float(np.float32(c.b1)), float(np.float32(c.b2)), float(C.ADAM_EPS), float(np.float32(c.gs)))
        ref = C.adam_reference(c, d)
        for k, t in (("p", p), ("m", m), ("v", v)):
            assert np.allclose(ref[k][0][s], t.numpy(), rtol=1e-12, atol=1e-300), (C.adam_id(c), k)


def test_adam_restatement_within_bounds():
    worst = 0.0
    for c in C.ADAM_CASES:
        d = C.adam_inputs(c)
        ref = C.adam_reference(c, d)
        for fused in (False, True):
            got = C.adam_f32(c, d, fused)
            got["g"] = d["g"]
            ratios, bad = C.adam_check(c, d, got, "value", ref)
            print(f"STEP-COVER-CPU {C.adam_id(c)} fused={int(fused)} restatement / bound " + " ".join(f"{k} {v:.3f}" for k, v in sorted(ratios.items())))
            assert not bad, (C.adam_id(c), fused, bad, ratios)
            worst = max(worst, *ratios.values())
    assert 0.02 < worst <= 1.0   # (a bound a hundred times the restatement's error would hold nothing)


def test_adam_cases_reach_every_edge():
    sizes = {c.n for c in C.ADAM_CASES}
    assert sizes == set(C.ADAM_SIZES) and len(C.ADAM_CASES) == len(C.ADAM_SIZES) * 6
    assert {n % 4 for n in sizes if n < 256} == {0, 1, 2, 3} == {n % 4 for n in sizes if n >= 256}
    assert any(n < 4 for n in sizes) and any(n >> 2 > 2 * 256 for n in sizes)   # no vector at all; several trips under the knob (2 blocks)
    assert {(c.b1, c.b2) for c in C.ADAM_CASES} == set(C.ADAM_BETAS) and {c.gs for c in C.ADAM_CASES} == set(C.ADAM_SCALES)
    for n in sizes:
        runs = C.adam_runs(n)
        assert (n >= 255) == bool(runs)
        if not runs:
            continue
        assert set(runs) == {"zero", "g0", "v0", "cancel", "denormal_v", "big_g"}
        d = C.adam_inputs(C.AdamCase(n, 0.9, 0.999, 0.5))
        tail = range(n - n % 4, n)
        assert any(s.start <= t < s.stop for s in runs["zero"] for t in tail) or n % 4 == 0   # an all-zero element in the scalar tail
        assert all((d[k][s] == 0).all() for s in runs["zero"] for k in "pgmv")
        assert (d["g"][runs["g0"][0]] == 0).all() and (d["v"][runs["g0"][0]] > 0).all()
        assert (d["v"][runs["v0"][0]] == 0).all() and (d["g"][runs["v0"][0]] != 0).all()
        s = runs["cancel"][0]
        t1, t2 = 0.9 * d["m"][s].astype(np.float64), 0.1 * 0.5 * d["g"][s].astype(np.float64)
        assert (np.abs(t1 + t2) < 1e-4 * np.abs(t1)).all()
        s = runs["denormal_v"][0]
        assert (d["v"][s] > 0).all() and (d["v"][s] < C.TINY).all() and (d["g"][s] == 0).any() and (d["g"][s] != 0).any()
        assert float(np.abs(d["g"][runs["big_g"][0]]).max()) == np.float32(1e15)


def test_adam_refusals(lib):
    P, st = 0x10000, None   # (never dereferenced: the argument checks come first)
    for fn, extra in ((lib.gs_adam_tf_step, (1e-3,)), (lib.gs_adam_tf_step_zero_grad, (1e-3,)), (lib.gs_adam_tf_step_dev, (P,))):
        tail = (0.0, 0.99, 1e-8, 1.0) + ((1, st) if fn is lib.gs_adam_tf_step_dev else (st,))
        for numel in (0, -5):
            assert fn(P, P, P, P, numel, *extra, *tail) == -1 and b"adam: numel must be positive" in lib.gs_last_error()
        for i in range(4):
            ptrs = [P] * 4
            ptrs[i] = None
            assert fn(*ptrs, 7, *extra, *tail) == -1 and b"adam: null pointer" in lib.gs_last_error(), i
            for off in (4, 8, 12):
                ptrs[i] = P + off
                assert fn(*ptrs, 7, *extra, *tail) == -1 and b"adam: pointers must be 16-byte aligned" in lib.gs_last_error(), (i, off)
    assert lib.gs_adam_tf_step_dev(P, P, P, P, 7, None, 0.0, 0.99, 1e-8, 1.0, 1, st) == -1 and b"lr_t_dev" in lib.gs_last_error()


# ---------------------------------------------------------------------------------------------------------------------------- losses
def _loss_autograd(c, d, kind, form):
    t = lambda a: torch.from_numpy(C.value64(a))
    lab = t(d["lab"])
    real, fake = t(d["real"]).requires_grad_(True), t(d["fake"]).requires_grad_(True)
    pen, ssq = t(d["pen"]).requires_grad_(True), t(d["ssq"]).requires_grad_(True)
    sp = lambda x: torch.nn.functional.softplus(x, threshold=1000.0)
    r, f = (real * lab).sum(dim=1), (fake * lab).sum(dim=1)
    if kind == "d":
        loss = ((sp(-r) if form != "fake" else 0.0) + (sp(f) if form != "real" else 0.0) + (float(C.PEN_W) * pen if form == "both+pen" else 0.0)).mean()
    else:
        loss = ((sp(-f) if form != "ssq" else 0.0) + (float(C.MS_W) / (ssq + float(C.MS_EPS)) if form != "fake" else 0.0)).mean()
    grads = torch.autograd.grad(loss, (real, fake, pen, ssq), allow_unused=True)
    return dict(zip(("loss", "g_real", "g_fake", "g_pen", "g_ssq"), [loss.detach().reshape(1)] + list(grads)))


def test_loss_reference_is_autograd_of_the_definition():
    n = 0
    for c in C.LOSS_CASES:
        if c.variant > 1 and c.n > 1:
            continue
        d = C.loss_inputs(c)
        for kind, form in C.loss_forms(c):
            ref, auto = C.loss_reference(c, d, kind, form), _loss_autograd(c, d, kind, form)
            for k, (r, _) in ref.items():
                assert auto[k] is not None and np.allclose(r, auto[k].numpy(), rtol=1e-11, atol=1e-300), (C.loss_id(c), kind, form, k)
            assert all(auto[k] is None for k in ("g_real", "g_fake", "g_pen", "g_ssq") if k not in ref)
            n += 1
    assert n > 100


def test_numpy_exp_and_log1p_are_within_what_the_bounds_assume():
    x = np.concatenate([np.linspace(-104, 21, 200001), np.array([0.0, 19.5, -19.5, 20.0, -20.5, 30, -30, 100, -100])]).astype(np.float32)
    with np.errstate(over="ignore", under="ignore"):
        e = np.exp(x)
        ok = np.isfinite(e) & (e >= C.TINY)
        assert (np.abs(e[ok].astype(np.float64) - np.exp(x[ok].astype(np.float64))) <= C.CPU_FN_U * C.U * np.exp(x[ok].astype(np.float64))).all()
        y = e[ok]
        assert (np.abs(np.log1p(y).astype(np.float64) - np.log1p(y.astype(np.float64))) <= C.CPU_FN_U * C.U * np.log1p(y.astype(np.float64))).all()
    assert C.FN_U == 4 * C.CPU_FN_U


def test_loss_restatement_within_bounds():
    worst = 0.0
    for c in C.LOSS_CASES:
        d = C.loss_inputs(c)
        for kind, form in C.loss_forms(c):
            ref = C.loss_reference(c, d, kind, form)
            for fused in (False, True):
                got = C.loss_f32(c, d, kind, form, fused)
                ratios, bad = C.loss_check(c, d, got, ref)
                print(f"STEP-COVER-CPU {C.loss_id(c)} {kind}:{form} fused={int(fused)} restatement / bound " + " ".join(f"{k} {v:.3f}" for k, v in sorted(ratios.items())))
                assert not bad, (C.loss_id(c), kind, form, fused, bad, ratios)
                worst = max(worst, *ratios.values())
    assert 0.02 < worst <= 1.0


def test_loss_cases_reach_every_edge():
    shapes = {(c.n, c.c) for c in C.LOSS_CASES}
    assert shapes == set(C.LOSS_SHAPES)
    assert {n % 4 for n, _ in shapes} == {0, 1, 2, 3} and any(n == 1 for n, _ in shapes) and any(256 < n < 1024 for n, _ in shapes) and any(n == 1024 for n, _ in shapes)
    assert any(64 < c <= 128 for _, c in shapes) and any(c > 128 for _, c in shapes) and any(c == 64 for _, c in shapes) and any(c == 1 for _, c in shapes)
    for dt in C.DTYPES:
        for n, cc in C.LOSS_SHAPES:
            seen_r, seen_f, classes = set(), set(), set()
            for c in (x for x in C.LOSS_CASES if (x.dtype, x.n, x.c) == (dt, n, cc)):
                d = C.loss_inputs(c)
                lab = C.value64(d["lab"])
                assert ((lab == 0) | (lab == 1)).all() and (lab.sum(axis=1) == 1).all()
                seen_r |= set((C.value64(d["real"]) * lab).sum(axis=1))
                seen_f |= set((C.value64(d["fake"]) * lab).sum(axis=1))
                classes |= set(d["cls"])
                assert d["ssq"].min() == 0.0 or n == 1
                assert d["ssq"].max() == np.float32(1e-3) or n == 1
            pins = {p for p in C.LOSS_PINS[dt] if p is not None}
            assert pins <= seen_r and pins <= seen_f, (dt, n, cc, sorted(pins - seen_r), sorted(pins - seen_f))   # every pin on both sides, at every shape
            assert len(seen_r - pins) > 0                                                                    # ... and plain draws
            assert {0, cc - 1} <= classes
    assert 100.0 in C.LOSS_PINS[C.F32] and 100.0 not in C.LOSS_PINS[C.BF16] and {0.0, 19.5, -19.5, 20.5, -20.5, 30.0, -30.0} <= set(C.LOSS_PINS[C.BF16])


def test_loss_refusals(lib):
    P, st = 0x10000, None
    d = lambda **kw: lib.gs_gan_d_loss(*[dict(dict(rl=P, fl=P, lab=P, pen=None, pw=1.0, n=8, c=61, loss=P, gr=P, gf=P, gp=None, dt=0, st=st), **kw)[k] for k in
                                         ("rl", "fl", "lab", "pen", "pw", "n", "c", "loss", "gr", "gf", "gp", "dt", "st")])
    g = lambda **kw: lib.gs_gan_g_loss(*[dict(dict(fl=P, lab=P, ssq=None, w=0.1, eps=1e-6, n=8, c=61, loss=P, gf=P, gs=None, dt=0, st=st, ), **kw)[k] for k in
                                         ("fl", "lab", "ssq", "w", "eps", "n", "c", "loss", "gf", "gs", "dt", "st")])
    for bad in (dict(n=0), dict(n=1025), dict(n=-1), dict(c=0), dict(rl=None, fl=None), dict(gr=None), dict(gf=None), dict(lab=None), dict(loss=None)):
        assert d(**bad) == -1 and b"gan_d_loss" in lib.gs_last_error(), bad
    for bad in (dict(n=0), dict(n=1025), dict(c=0), dict(fl=None), dict(gf=None), dict(lab=None), dict(loss=None), dict(ssq=P), dict(fl=None, ssq=P, gs=None)):
        assert g(**bad) == -1 and b"gan_g_loss" in lib.gs_last_error(), bad


# ------------------------------------------------------------------------------------------------------------------------- embedding
def test_embedding_reference_is_autograd_of_an_index_select():
    for c in C.EMB_CASES:
        d = C.emb_inputs(c)
        w = torch.from_numpy(d["w"].astype(np.float64)).requires_grad_(True)
        y = w.index_select(0, torch.from_numpy(d["idx"])) * float(C.EMB_ALPHA)
        (gw,) = torch.autograd.grad(y, w, torch.from_numpy(C.value64(d["gy"])))
        ref, bound, unselected = C.emb_backward_reference(c, d)
        assert np.allclose(ref, gw.numpy(), rtol=1e-12, atol=1e-300) and (ref[unselected] == 0).all() and (bound[unselected] == 0).all()
        assert np.array_equal(C.first_max(d["lab"]), torch.argmax(torch.from_numpy(C.value64(d["lab"])), dim=1).numpy()), C.emb_id(c)
        fwd = C.value64(C.emb_forward_bits(c, d["w"], d["idx"]))
        assert np.allclose(fwd, y.detach().numpy(), rtol=2.0 ** -8 if c.dtype == C.BF16 else 2.0 ** -23, atol=0)
        worst = _margin(C.emb_id(c), "gw", C.emb_backward_f32(c, d), ref, bound)
        assert worst <= 1.0


def test_embedding_cases_reach_every_edge():
    shapes = {(c.b, c.rows, c.units) for c in C.EMB_CASES}
    assert shapes == set(C.EMB_SHAPES)
    assert any(r > 256 for _, r, _ in shapes) and any(u > 256 for _, _, u in shapes) and any(u % 256 and u > 1 for _, _, u in shapes) and (1, 1, 1) in shapes
    assert any(b * u > 256 for b, _, u in shapes) and any(r * u > 256 for _, r, u in shapes)   # more than one block of the gathers
    for dt in C.DTYPES:
        unselected = repeated = same_thread_tie = all_equal_long = 0
        for b, r, u in C.EMB_SHAPES:
            patterns = set()
            for c in (x for x in C.EMB_CASES if (x.dtype, x.b, x.rows, x.units) == (dt, b, r, u)):
                d = C.emb_inputs(c)
                lab, first = C.value64(d["lab"]), C.first_max(d["lab"])
                assert d["idx"][0] == 0 and (b < 2 or d["idx"][1] == r - 1)
                assert {-1, r} >= set(d["clamp_idx"]) - set(range(r)) and len(set(d["clamp_idx"]) - set(range(r))) == min(b, 2)
                unselected += len(C.emb_backward_reference(c, d)[2]) > 0
                repeated += len(set(d["idx"])) < b
                for i in range(b):
                    pat = C.emb_pattern(c, i)
                    patterns.add(pat)
                    row = lab[i]
                    if pat == "tie" and r > 1:
                        assert (row == row.max()).sum() == 2 and first[i] == np.flatnonzero(row == row.max())[0] and row[d["idx"][i]] == row.max()
                        same_thread_tie += int(np.flatnonzero(row == row.max())[1] - first[i] == 256)
                    if pat == "all_equal":
                        assert first[i] == 0
                        all_equal_long += r > 256
                    if pat == "last":
                        assert first[i] == r - 1
                    if pat == "minus_inf":
                        assert np.isneginf(row).sum() == r - 1 and first[i] == d["idx"][i]
                    if pat == "onehot":
                        assert row.sum() == 1 and first[i] == d["idx"][i]
            assert patterns == set(C.EMB_PATTERNS), (dt, b, r, u)
        assert unselected and repeated and same_thread_tie and all_equal_long, (unselected, repeated, same_thread_tie, all_equal_long)


def test_embedding_refusals(lib):
    P, st = 0x10000, None
    for b, r, u in ((0, 5, 7), (3, 0, 7), (3, 5, 0), (-1, 5, 7), (3, -5, 7), (3, 5, -7)):
        assert lib.gs_embedding_fwd(P, P, P, b, r, u, 1.0, 0, st) == -1 and b"embedding_fwd" in lib.gs_last_error()
        assert lib.gs_embedding_bwd(P, P, P, b, r, u, 1.0, 0, st) == -1 and b"embedding_bwd" in lib.gs_last_error()
        assert lib.gs_embedding_onehot_fwd(P, P, P, P, b, r, u, 1.0, 0, st) == -1 and b"embedding_onehot_fwd" in lib.gs_last_error()
    for i in range(4):
        ptrs = [P] * 4
        ptrs[i] = None
        assert lib.gs_embedding_onehot_fwd(*ptrs, 3, 5, 7, 1.0, 0, st) == -1 and b"embedding_onehot_fwd" in lib.gs_last_error(), i


# ----------------------------------------------------------------------------------------------------------------------- weight prep
def test_prep_layouts_are_transpose_flip_and_copy():
    for c in C.PREP_CASES:
        if c.ci * c.co > 96 * 160:
            continue
        w = C.prep_weight(c)
        variant, f32 = C.prep_plan(c)
        exp = C.prep_expected(c, w)
        k, taps = c.ksize, c.ksize * c.ksize
        want = np.zeros((taps, c.co, c.ci) if variant == 0 else (taps, c.ci, c.co), dtype=np.float32)
        for t in range(taps):
            ky, kx = divmod(t, k)
            if variant == 0:
                want[t] = w[ky, kx].transpose(1, 0)
            elif variant == 1:
                want[t] = w[k - 1 - ky, k - 1 - kx]   # the kernel turned by 180 degrees
            else:
                want[t] = w[ky, kx]
        assert exp.shape == want.shape and exp.dtype == (np.float32 if f32 else np.uint16)
        assert C.same_bits(exp, want if f32 else torch.from_numpy(want).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)), C.prep_id(c)


def test_prep_cases_reach_every_edge(lib):
    from gansynth_amd import _lib
    facts = {c: C.prep_facts(c) for c in C.PREP_CASES}
    has = lambda **kw: any(all((getattr(c, k) if hasattr(c, k) else f[k]) == v for k, v in kw.items()) for c, f in facts.items())
    assert len(set(C.PREP_CASES)) == len(C.PREP_CASES) > 30
    for dt in C.DTYPES:
        assert has(map=C.PREP_FWD, ci=32, co=32, ksize=3, dtype=dt, f32=(dt == C.F32))
        for variant in (0, 1, 2):
            assert has(variant=variant, dtype=dt, partial_ci=True, partial_co=True) and has(variant=variant, dtype=dt, scalar_read=True, scalar_write=True)
            assert has(variant=variant, dtype=dt, f32=True)
        assert has(map=C.PREP_FWD, ci=1, co=16, dtype=dt) and has(ksize=1, ci=32, co=2, dtype=dt, f32=True) and has(ksize=1, ci=2, co=32, dtype=dt, f32=True)
        assert has(map=C.PREP_BWD_DATA, stride=1, variant=1, dtype=dt) and has(map=C.PREP_BWD_DATA, stride=2, variant=2, dtype=dt)
        assert has(map=C.PREP_T_FWD, ci=64, co=32, variant=0, dtype=dt) and has(map=C.PREP_T_BWD_DATA, ci=64, co=32, variant=2, dtype=dt)
    for variant in (0, 1, 2):   # bf16 storage: whole tiles, and partial ones
        assert has(variant=variant, dtype=C.BF16, f32=False) and (variant == 1 or has(variant=variant, dtype=C.BF16, f32=False, partial_ci=True, partial_co=True))
    assert has(map=C.PREP_FWD, ci=256, co=256, dtype=C.BF16, tiles=144, trips=3, f32=False)
    assert has(map=C.PREP_FWD, ci=16, co=32, dtype=C.F32) and has(map=C.PREP_BWD_DATA, ci=16, co=32, dtype=C.F32)
    assert C.igemm_supported(16, 32, C.F32) and not C.igemm_supported(32, 16, C.F32)
    assert {f["trips"] for f in facts.values()} >= {1, 2, 3}
    # the operand fits the workspace the library asks for, and the storage restated here is the one the conv entry points read: an MFMA-eligible
    # bf16 layer's operand is half the fp32 size
    for c in C.PREP_CASES:
        conv = _lib.GsConv(2, 4, 8, c.ci, c.co, c.ksize, c.stride, 1 if c.map in (C.PREP_T_FWD, C.PREP_T_BWD_DATA) else 0, c.dtype, 0, 1.0, None, 0)
        nb = lib.gs_conv_workspace_bytes(conv, _lib.CONV_FWD if c.map in (C.PREP_FWD, C.PREP_T_FWD) else _lib.CONV_BWD_DATA)
        assert 0 < C.prep_expected(c, C.prep_weight(c)).nbytes <= nb, C.prep_id(c)
    assert {(k, ci, co) for k, ci, co, *_ in C.PROMISE_LAYERS} == {(3, 32, 32), (3, 6, 40), (1, 32, 2)}


def test_prep_refusals(lib):
    P = 0x10000
    for table, n in ((None, 3), (P, 0), (P, -1), (P, 65536)):
        assert lib.gs_weight_prep_batch(table, n, None) == -1 and b"weight_prep_batch" in lib.gs_last_error(), (table, n)
