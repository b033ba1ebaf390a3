"""The cases of the kernels that run every iteration outside the route-driven covers -- TF-Adam (csrc/elementwise.hip: adam_tf_kernel<ZERO, DEV>), the
two GAN losses and the three embedding kernels (csrc/small_ops.hip) and the batched weight re-layout (csrc/conv_api.hip: weight_prep_batch_kernel) --
shared by tests/test_step_cover_cpu.py and tests/test_step_cover_gpu.py (a plain helper module: no fixtures, no collection hooks).

Every reference is float64 on the operands AS STORED (fp32 scalars as the kernel receives them, activations rounded to bf16 for bf16).  Every bound
counts roundings; u = 2^-24 is the unit round-off of fp32, a count is doubled (a factor 2 of margin, never more), 2^-149 is the denormal quantum.

Adam, per element, gr = g * gs, m' = b1 m + (1 - b1) gr, v' = b2 v + ((1 - b2) gr) gr, p' = p - (lr_t m') / (sqrt(v') + eps):
  m'  4 roundings (gr, 1 - b1, their product, b1 m or the sum: the larger path): |m' - ref| <= 2 * 4 u (|b1 m| + |(1 - b1) g gs|) + 4 * 2^-149
  v'  6 roundings (gr twice, 1 - b2, two products, b2 v / the sum), every term non-negative:  |v' - ref| <= 2 * 6 u v' + 4 * 2^-149
  p'  the subtraction (1, of |p'|) and the step: lr_t m', sqrtf, + eps, the division (4; sqrtf and the division are correctly rounded) and half
      the relative error of v' under the root (3): |p' - ref| <= 2 u (|p'| + 7 |step|) + lr_t (bound of m') / (sqrt(v') + eps)
  |g| beyond 1e15 is left out: g * g overflows fp32 there, as it does in TensorFlow, and a float64 reference says nothing about it.
Losses.  No document of the device library that states the error of expf / log1pf comes with the toolchain; as tests/reverb_ref.py does, the bound
takes the functions of the CPU restatement (numpy's fp32 exp and log1p: within 3 ulp = 6 u, numpy's documented worst case rounded up, asserted in the
CPU file) with a factor 4: FN_U = 24 u per call.
  loss     n-term fp32 summation, (n - 1) u, 5 roundings around it (two additions and a product inside a sample, 1 / n and the product with it), doubled,
           and 2 FN_U of softplus = log1pf(expf(.)) per term, all relative to the mean of the terms' magnitudes; + 2^-126 (a term below the smallest
           normal number has no relative accuracy, and expf may flush it)
  g_logit  4 roundings (1 + e, the reciprocal, 1 / n, the product; the label is 0 or 1) doubled + FN_U of expf: 32 u |ref| + u / n, exactly 0 where
           the label is 0; bf16 results: + 2^-8 |ref| (the one rounding of the store: 8 significant bits)
  g_pen    2 roundings: 4 u |ref|;   g_sumsq  6 (s + eps counts twice under the square, d d, w / ., 1 / n, the product): 12 u |ref|
Embedding: the forward is the fp32 product w[idx] * alpha rounded to the dtype, bit for bit; the backward b u alpha sum |gy| over the samples of
the row, exactly 0 for a row no sample selects.  Weight prep: bytes.
"""
from collections import namedtuple

import numpy as np
import torch

U = 2.0 ** -24
DENORMAL = 2.0 ** -149
TINY = 2.0 ** -126
CPU_FN_U, FN_U = 6, 24   # relative error of an exp / log1p call in units of u: the CPU restatement's, and four times it for the device
F32, BF16 = 0, 1
DTYPES = (F32, BF16)
DTYPE_NAMES = ("f32", "bf16")
KNOBS = {"GS_EW_GRID_CAP": "2"}   # the child of the GPU test: two blocks, so 64003 elements are 32 trips of the grid-stride loop
GUARD, GUARD_BYTE, POISON_BYTE = 256, 0xA5, 0xCD


# ----------------------------------------------------------------------------------------------------------------- bf16 as bits
def bf16_bits(a):
    """fp32 values -> bf16 bit patterns (uint16), round to nearest even as torch.bfloat16 rounds."""
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16)
    return t.view(torch.int16).numpy().view(np.uint16).copy()


def bf16_value(bits):
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def stored(a, dtype):
    """The array as a kernel stores it: fp32, or bf16 bits."""
    return np.ascontiguousarray(a, dtype=np.float32) if dtype == F32 else bf16_bits(a)


def value64(a):
    """float64 values of a stored array (fp32, or bf16 bits)."""
    return (bf16_value(a) if a.dtype == np.uint16 else a).astype(np.float64)


# --------------------------------------------------------------------------------------------------------------- guarded buffers
def guarded(a):
    """A device byte buffer with GUARD bytes of a known pattern on either side of the bytes of `a`."""
    raw = np.frombuffer(np.ascontiguousarray(a).tobytes(), dtype=np.uint8).copy()
    buf = torch.full((2 * GUARD + raw.size,), GUARD_BYTE, dtype=torch.uint8, device="cuda")
    buf[GUARD:GUARD + raw.size] = torch.from_numpy(raw).cuda()
    return buf


def poisoned(shape, np_dtype):
    """A guarded OUTPUT buffer: every byte the kernel does not write stays recognisable."""
    return guarded(np.full(int(np.prod(shape)) * np.dtype(np_dtype).itemsize, POISON_BYTE, dtype=np.uint8))


def ptr(buf):
    return buf.data_ptr() + GUARD   # (torch allocations are 512-byte aligned, GUARD keeps 16)


def payload(buf, np_dtype, shape=None):
    a = buf[GUARD:buf.numel() - GUARD].cpu().numpy().view(np_dtype)
    return a if shape is None else a.reshape(shape)


def guards_intact(buf):
    return bool((buf[:GUARD] == GUARD_BYTE).all()) and bool((buf[buf.numel() - GUARD:] == GUARD_BYTE).all())


def f32_view(buf):
    return buf[GUARD:buf.numel() - GUARD].view(torch.float32)


def _stream():
    from gansynth_amd import kernels
    return kernels._stream()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# =============================================================================================================================== Adam
ADAM_SIZES = (1, 2, 3, 4, 5, 7, 255, 256, 257, 1023, 1026, 64003)
ADAM_BETAS = ((0.0, 0.99), (0.5, 0.99), (0.9, 0.999))
ADAM_SCALES = (1.0, 0.5)
ADAM_ENTRIES = ("value", "zero", "dev", "dev_zero")   # gs_adam_tf_step, gs_adam_tf_step_zero_grad, gs_adam_tf_step_dev with zero_grad 0 / 1
ADAM_LR_T, ADAM_EPS = np.float32(1.0e-3), np.float32(1.0e-8)
ADAM_SKIP_SIZES = (3, 257)   # a negative device scalar: nothing moves
AdamCase = namedtuple("AdamCase", "n b1 b2 gs")
ADAM_CASES = [AdamCase(n, b1, b2, gs) for n in ADAM_SIZES for b1, b2 in ADAM_BETAS for gs in ADAM_SCALES]


def adam_runs(n):
    """name -> slices: the special stretches of a buffer of n >= 255 elements (everything else: normal draws with v >= 0)."""
    if n < 255:
        return {}
    return {"zero": [slice(0, 32), slice(n - 2, n)], "g0": [slice(32, 64)], "v0": [slice(64, 96)], "cancel": [slice(96, 128)],
            "denormal_v": [slice(128, 160)], "big_g": [slice(160, 192)]}


def adam_inputs(c):
    rng = np.random.default_rng(1000 + c.n)
    f = np.float32
    p, g, m = (rng.standard_normal(c.n).astype(f) for _ in range(3))
    v = (0.1 * rng.standard_normal(c.n) ** 2).astype(f)
    runs = adam_runs(c.n)
    for s in runs.get("zero", []):
        p[s] = g[s] = m[s] = v[s] = 0.0
    for s in runs.get("g0", []):
        g[s] = 0.0
    for s in runs.get("v0", []):
        v[s] = 0.0
    for s in runs.get("cancel", []):
        if c.b1 > 0:   # b1 m = -(1 - b1) g gs (1 + k 2^-20): the sum is 2^-20 .. 2^-15 of its terms
            k = np.arange(1, s.stop - s.start + 1)
            m[s] = (-(1.0 - float(f(c.b1))) * g[s].astype(np.float64) * float(f(c.gs)) / float(f(c.b1)) * (1.0 + k * 2.0 ** -20)).astype(f)
    for s in runs.get("denormal_v", []):
        k = np.arange(1, s.stop - s.start + 1)
        v[s] = (k * DENORMAL).astype(f)
        g[s.start:s.start + 16] = 0.0
    for s in runs.get("big_g", []):
        k = s.stop - s.start
        g[s] = (np.where(np.arange(k) % 2 == 0, 1.0, -1.0) * 10.0 ** np.linspace(5.0, 15.0, k)).astype(f)
    assert bool((v >= 0).all()) and float(np.abs(g).max()) <= 1.0e15
    return {"p": p, "g": g, "m": m, "v": v}


def _adam_scalars(c):
    f = np.float32
    return f(c.b1), f(c.b2), f(c.gs)


def adam_reference(c, d, lr_t=ADAM_LR_T):
    """name -> (float64 result, bound per element) for m, v, p."""
    b1, b2, gs = (float(x) for x in _adam_scalars(c))
    lr, eps = float(lr_t), float(ADAM_EPS)
    p, g, m, v = (d[k].astype(np.float64) for k in "pgmv")
    t1, t2 = b1 * m, (1.0 - b1) * g * gs
    m1 = t1 + t2
    v1 = b2 * v + (1.0 - b2) * (g * gs) ** 2
    den = np.sqrt(v1) + eps
    step = lr * m1 / den
    p1 = p - step
    bm = 2 * 4 * U * (np.abs(t1) + np.abs(t2)) + 4 * DENORMAL
    bv = 2 * 6 * U * v1 + 4 * DENORMAL
    bp = 2 * U * (np.abs(p1) + 7 * np.abs(step)) + lr * bm / den
    return {"m": (m1, bm), "v": (v1, bv), "p": (p1, bp)}


def _fma(a, b, c):
    """fmaf, emulated: the product of two fp32 numbers is exact in float64; one rounding to fp32 behind the sum."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def adam_f32(c, d, fused, lr_t=ADAM_LR_T):
    """The kernel's arithmetic in fp32 numpy, with the multiply-adds fused or not."""
    f = np.float32
    b1, b2, gs = _adam_scalars(c)
    p, g, m, v = (d[k] for k in "pgmv")
    with np.errstate(under="ignore"):
        gr = g * gs
        if fused:
            m1 = _fma(np.full_like(gr, f(1) - b1), gr, b1 * m)
            v1 = _fma((f(1) - b2) * gr, gr, b2 * v)
        else:
            m1 = b1 * m + (f(1) - b1) * gr
            v1 = b2 * v + (f(1) - b2) * gr * gr
        p1 = p - f(lr_t) * m1 / (np.sqrt(v1) + ADAM_EPS)
    return {"m": m1.astype(f), "v": v1.astype(f), "p": p1.astype(f)}


def adam_run(K, c, d, entry, lr_t=ADAM_LR_T):
    """One entry point on guarded copies of the four buffers: name -> fp32 array afterwards (guards checked)."""
    bufs = {k: guarded(d[k]) for k in "pgmv"}
    views = [f32_view(bufs[k]) for k in "pgmv"]
    assert all(t.numel() == c.n and t.data_ptr() % 16 == 0 for t in views)
    args = (float(np.float32(c.b1)), float(np.float32(c.b2)), float(ADAM_EPS), float(np.float32(c.gs)))
    if entry in ("value", "zero"):
        K.adam_tf_step(*views, float(lr_t), *args, refresh=False, zero_grad=entry == "zero")
    else:
        scalar = torch.tensor([float(lr_t)], dtype=torch.float32, device="cuda")
        K.adam_tf_step_dev(*views, scalar.data_ptr(), *args, refresh=False, zero_grad=entry == "dev_zero")
    torch.cuda.synchronize()
    assert all(guards_intact(b) for b in bufs.values()), ("guard words", adam_id(c), entry)
    return {k: payload(bufs[k], np.float32) for k in "pgmv"}


def adam_id(c):
    return f"adam n={c.n} b1={c.b1} b2={c.b2} gs={c.gs}"


def adam_check(c, d, got, entry, ref=None):
    """-> ({name: worst |error| / bound}, [failures]) of one entry point's results."""
    ref = ref or adam_reference(c, d)
    ratios, bad = {}, []
    for k in "mvp":
        r, b = ref[k]
        err = np.abs(got[k].astype(np.float64) - r)
        ratios[k] = float(np.max(np.where(err == 0, 0.0, err / np.maximum(b, 1e-300))))
        if not bool((err <= b).all()) or not bool(np.isfinite(got[k]).all()):
            bad.append(k)
    if entry in ("zero", "dev_zero"):
        if not same_bits(got["g"], np.zeros(c.n, dtype=np.float32)):
            bad.append("g not +0.0 everywhere")
    elif not same_bits(got["g"], d["g"]):
        bad.append("g changed")
    for s in adam_runs(c.n).get("zero", []):
        for k in "pmv":
            if not same_bits(got[k][s], np.zeros(s.stop - s.start, dtype=np.float32)):
                bad.append(f"all-zero run: {k} is not +0.0")
    return ratios, bad


# ========================================================================================================================== GAN losses
LOSS_SHAPES = ((1, 1), (1, 61), (3, 61), (5, 64), (6, 65), (8, 130), (257, 61), (1024, 3))
LOSS_PINS = {F32: (None, 0.0, 19.5, -19.5, 20.5, -20.5, 30.0, -30.0, 100.0, -100.0), BF16: (None, 0.0, 19.5, -19.5, 20.5, -20.5, 30.0, -30.0)}
D_FORMS = ("both+pen", "both", "real", "fake")
G_FORMS = ("fake+ssq", "fake", "ssq")
PEN_W, MS_W, MS_EPS = np.float32(2.5), np.float32(0.1), np.float32(1.0e-6)
LossCase = namedtuple("LossCase", "dtype n c variant")   # variant: which stretch of the pin list the first samples take
LOSS_CASES = [LossCase(dt, n, c, v) for dt in DTYPES for n, c in LOSS_SHAPES for v in range(-(-len(LOSS_PINS[dt]) // n))]


def loss_id(c):
    return f"loss-{DTYPE_NAMES[c.dtype]} {c.n}x{c.c} v{c.variant}"


def loss_inputs(c):
    rng = np.random.default_rng(2000 + 7 * c.n + c.c)
    pins = LOSS_PINS[c.dtype]
    real, fake = (3.0 * rng.standard_normal((c.n, c.c))).astype(np.float32), (3.0 * rng.standard_normal((c.n, c.c))).astype(np.float32)
    draws = rng.integers(0, c.c, c.n)
    cls = np.zeros(c.n, dtype=np.int64)
    for i in range(c.n):
        base = i + c.variant * c.n
        cls[i] = (0, c.c - 1, draws[i])[base % 3]
        pin_r, pin_f = (pins[base], pins[len(pins) - 1 - base]) if base < len(pins) else (None, None)   # (the fake side walks the list backwards)
        if pin_r is not None:
            real[i, cls[i]] = pin_r
        if pin_f is not None:
            fake[i, cls[i]] = pin_f
    lab = np.zeros((c.n, c.c), dtype=np.float32)
    lab[np.arange(c.n), cls] = 1.0
    pen = (2.0 * rng.random(c.n)).astype(np.float32)
    ssq = (1.0e-3 * (np.arange(c.n) / max(c.n - 1, 1)) ** 2).astype(np.float32) if c.n > 1 else np.array([(0.0, 1.0e-3, 1.0e-6)[c.variant % 3]], dtype=np.float32)
    return {"real": stored(real, c.dtype), "fake": stored(fake, c.dtype), "lab": stored(lab, c.dtype), "pen": pen, "ssq": ssq, "cls": cls}


def _softplus64(x):
    return np.logaddexp(0.0, x)


def _sigmoid64(x):
    return np.exp(-np.logaddexp(0.0, -x))


def loss_reference(c, d, kind, form):
    """name -> (float64 result, bound): 'loss', and the gradients the form writes."""
    n = c.n
    lab = value64(d["lab"])
    out = {}
    terms = np.zeros(n)

    def logit_grad(g):
        b = (2 * 4 + FN_U) * U * np.abs(g) + U / n
        return g, (b + 2.0 ** -8 * np.abs(g) if c.dtype == BF16 else b)
    if kind == "d":
        if form != "fake":
            r = (value64(d["real"]) * lab).sum(axis=1)
            terms = terms + _softplus64(-r)
            out["g_real"] = logit_grad(-_sigmoid64(-r)[:, None] / n * lab)
        if form != "real":
            f = (value64(d["fake"]) * lab).sum(axis=1)
            terms = terms + _softplus64(f)
            out["g_fake"] = logit_grad(_sigmoid64(f)[:, None] / n * lab)
        if form == "both+pen":
            terms = terms + float(PEN_W) * d["pen"].astype(np.float64)
            gp = np.full(n, float(PEN_W) / n)
            out["g_pen"] = (gp, 4 * U * np.abs(gp))
    else:
        if form != "ssq":
            f = (value64(d["fake"]) * lab).sum(axis=1)
            terms = terms + _softplus64(-f)
            out["g_fake"] = logit_grad(-_sigmoid64(-f)[:, None] / n * lab)
        if form != "fake":
            dd = d["ssq"].astype(np.float64) + float(MS_EPS)
            terms = terms + float(MS_W) / dd
            gs = -float(MS_W) / (dd * dd) / n
            out["g_ssq"] = (gs, 12 * U * np.abs(gs))
    assert bool((terms >= 0).all())
    loss = terms.sum() / n
    out["loss"] = (np.array([loss]), np.array([(2 * (n - 1 + 5) + 2 * FN_U) * U * loss + TINY]))
    return out


def _softplus32(x):
    f = np.float32
    with np.errstate(over="ignore", under="ignore"):
        return np.where(x > f(20), x, np.log1p(np.exp(x.astype(f)))).astype(f)


def _sigmoid32(x):
    f = np.float32
    with np.errstate(over="ignore", under="ignore"):
        return (f(1) / (f(1) + np.exp((-x).astype(f)))).astype(f)


def _wave_order_sum(terms):
    """The kernel's order: wave w adds samples w, w + 4, ... one after the other; then the four partial sums."""
    f = np.float32
    part = np.zeros(4, dtype=f)
    pad = np.zeros(-(-len(terms) // 4) * 4, dtype=f)
    pad[:len(terms)] = terms
    for row in pad.reshape(-1, 4):
        part = part + row
    return f(f(part[0] + part[1]) + f(part[2] + part[3]))


def loss_f32(c, d, kind, form, fused):
    """The kernels' arithmetic in fp32 numpy (the same names as loss_reference; logit gradients before the store's rounding)."""
    f = np.float32
    n = c.n
    inv_n = f(1) / f(n)
    lab = value64(d["lab"]).astype(f)
    out = {}
    terms = np.zeros(n, dtype=f)
    if kind == "d":
        if form != "fake":
            r = (value64(d["real"]) * lab).sum(axis=1).astype(f)   # (one non-zero product per sample: exact)
            terms = terms + _softplus32(-r)
            out["g_real"] = (-_sigmoid32(-r) * inv_n)[:, None] * lab
        if form != "real":
            fl = (value64(d["fake"]) * lab).sum(axis=1).astype(f)
            terms = terms + _softplus32(fl)
            out["g_fake"] = (_sigmoid32(fl) * inv_n)[:, None] * lab
        if form == "both+pen":
            terms = _fma(np.full(n, PEN_W), d["pen"], terms) if fused else terms + PEN_W * d["pen"]
            out["g_pen"] = np.full(n, PEN_W * inv_n, dtype=f)
    else:
        if form != "ssq":
            fl = (value64(d["fake"]) * lab).sum(axis=1).astype(f)
            terms = terms + _softplus32(-fl)
            out["g_fake"] = (-_sigmoid32(-fl) * inv_n)[:, None] * lab
        if form != "fake":
            dd = d["ssq"] + MS_EPS
            terms = terms + MS_W / dd
            out["g_ssq"] = (-MS_W / (dd * dd) * inv_n).astype(f)
    out["loss"] = np.array([_wave_order_sum(terms.astype(f)) * inv_n], dtype=f)
    if c.dtype == BF16:
        for k in ("g_real", "g_fake"):
            if k in out:
                out[k] = bf16_bits(out[k])
    return out


def loss_run(K, c, d, kind, form):
    """One launch through K.lib on guarded buffers: name -> stored array (fp32, or bf16 bits for the logit gradients of a bf16 case)."""
    n, cc = c.n, c.c
    act = np.float32 if c.dtype == F32 else np.uint16
    ins = {k: guarded(d[k]) for k in ("real", "fake", "lab", "pen", "ssq")}
    outs = {"loss": poisoned((1,), np.float32)}
    want_real, want_fake = kind == "d" and form != "fake", form not in ("real", "ssq")
    if want_real:
        outs["g_real"] = poisoned((n, cc), act)
    if want_fake:
        outs["g_fake"] = poisoned((n, cc), act)

    def p(name, table=ins):
        return ptr(table[name]) if name in table else None
    if kind == "d":
        if form == "both+pen":
            outs["g_pen"] = poisoned((n,), np.float32)
        rc = K.lib.gs_gan_d_loss(p("real") if want_real else None, p("fake") if want_fake else None, p("lab"), p("pen") if form == "both+pen" else None, float(PEN_W),
                                 n, cc, p("loss", outs), p("g_real", outs), p("g_fake", outs), p("g_pen", outs), c.dtype, _stream())
    elif form == "ssq":   # the mode-seeking half alone, as kernels.gan_g_loss calls it: c = 1, fp32
        outs["g_ssq"] = poisoned((n,), np.float32)
        rc = K.lib.gs_gan_g_loss(None, None, p("ssq"), float(MS_W), float(MS_EPS), n, 1, p("loss", outs), None, p("g_ssq", outs), F32, _stream())
    else:
        if form == "fake+ssq":
            outs["g_ssq"] = poisoned((n,), np.float32)
        rc = K.lib.gs_gan_g_loss(p("fake"), p("lab"), p("ssq") if form == "fake+ssq" else None, float(MS_W), float(MS_EPS), n, cc, p("loss", outs), p("g_fake", outs),
                                 p("g_ssq", outs), c.dtype, _stream())
    assert rc == 0, (rc, K.lib.gs_last_error())
    torch.cuda.synchronize()
    assert all(guards_intact(b) for b in list(ins.values()) + list(outs.values())), ("guard words", loss_id(c), kind, form)
    for k in ins:   # what a kernel only reads keeps its bits
        assert same_bits(payload(ins[k], d[k].dtype, d[k].shape), d[k]), ("input changed", loss_id(c), kind, form, k)
    return {k: payload(b, act if k in ("g_real", "g_fake") else np.float32, (n, cc) if k in ("g_real", "g_fake") else None) for k, b in outs.items()}


def loss_check(c, d, got, ref):
    """-> ({name: worst |error| / bound}, [failures])."""
    ratios, bad = {}, []
    lab = value64(d["lab"])
    assert set(got) == set(ref), (sorted(got), sorted(ref))
    for k, (r, b) in ref.items():
        g = value64(got[k])
        err = np.abs(g - r)
        ratios[k] = float(np.max(np.where(err == 0, 0.0, err / np.maximum(b, 1e-300))))
        if not bool((err <= b).all()) or not bool(np.isfinite(g).all()):
            bad.append(k)
        if k in ("g_real", "g_fake") and not bool((g[lab == 0] == 0).all()):
            bad.append(k + " off the label")
    return ratios, bad


# =========================================================================================================================== embedding
EMB_SHAPES = ((1, 1, 1), (3, 5, 7), (8, 61, 256), (5, 300, 33), (9, 61, 300), (64, 61, 256))
EMB_ALPHA = np.float32(np.sqrt(2.0 / 256.0))
EMB_PATTERNS = ("onehot", "tie", "all_equal", "last", "minus_inf")
EmbCase = namedtuple("EmbCase", "dtype b rows units variant")   # variant: rotates the label patterns over the samples
EMB_CASES = [EmbCase(dt, b, r, u, v) for dt in DTYPES for b, r, u in EMB_SHAPES for v in range(len(EMB_PATTERNS))]


def emb_id(c):
    return f"embedding-{DTYPE_NAMES[c.dtype]} {c.b}x{c.rows}x{c.units} v{c.variant}"


def emb_pattern(c, i):
    return EMB_PATTERNS[(i + c.variant) % len(EMB_PATTERNS)]


def emb_inputs(c):
    rng = np.random.default_rng(3000 + 11 * c.b + c.rows + c.units)
    w = rng.standard_normal((c.rows, c.units)).astype(np.float32)
    idx = np.zeros(c.b, dtype=np.int64)
    for i in range(c.b):   # 0, rows - 1, a draw, and that draw once more
        idx[i] = (0, c.rows - 1, rng.integers(0, c.rows), idx[i - 1])[i % 4]
    clamp_idx = idx.copy()
    clamp_idx[0] = (-1, c.rows)[c.variant % 2]
    if c.b > 1:
        clamp_idx[-1] = (c.rows, -1)[c.variant % 2]
    lab = np.zeros((c.b, c.rows), dtype=np.float32)
    for i in range(c.b):
        pat, k = emb_pattern(c, i), int(idx[i])
        if pat == "onehot":
            lab[i, k] = 1.0
        elif pat == "tie":   # a second maximum: 256 behind the first where the row is that long (the same thread's next trip), else next to it, else at 0
            lab[i] = 0.25 * rng.random(c.rows)
            lab[i, k] = 1.0
            lab[i, k + 256 if k + 256 < c.rows else (k + 1 if k + 1 < c.rows else 0)] = 1.0
        elif pat == "all_equal":
            lab[i] = 0.5
        elif pat == "last":
            lab[i] = 0.5 * rng.random(c.rows)
            lab[i, c.rows - 1] = 1.0
        else:
            lab[i] = -np.inf
            lab[i, k] = -3.0
    gy = rng.standard_normal((c.b, c.units)).astype(np.float32)
    return {"w": w, "idx": idx, "clamp_idx": clamp_idx, "lab": stored(lab, c.dtype), "gy": stored(gy, c.dtype)}


def first_max(lab):
    """The first maximum of every row of the stored labels, written out: the index the one-hot forward must choose."""
    v = value64(lab)
    out = np.zeros(v.shape[0], dtype=np.int64)
    for i, row in enumerate(v):
        best, bi = -np.inf, 0
        for k, x in enumerate(row):
            if x > best:
                best, bi = x, k
        out[i] = bi
    return out


def emb_forward_bits(c, w, idx):
    """w[clamped idx] * alpha: one fp32 product, stored in the dtype."""
    k = np.clip(idx, 0, c.rows - 1)
    return stored(w[k] * EMB_ALPHA, c.dtype)


def emb_backward_reference(c, d, idx=None):
    """(float64 gw, bound per element, rows no sample selects)."""
    idx = d["idx"] if idx is None else idx
    gy = value64(d["gy"])
    gw, mag = np.zeros((c.rows, c.units)), np.zeros((c.rows, c.units))
    for i, k in enumerate(idx):
        gw[k] += gy[i]
        mag[k] += np.abs(gy[i])
    unselected = np.setdiff1d(np.arange(c.rows), idx)
    return gw * float(EMB_ALPHA), c.b * U * float(EMB_ALPHA) * mag, unselected


def emb_backward_f32(c, d):
    f = np.float32
    gy = value64(d["gy"]).astype(f)
    gw = np.zeros((c.rows, c.units), dtype=f)
    for i, k in enumerate(d["idx"]):
        gw[k] = gw[k] + gy[i]
    return gw * EMB_ALPHA


def emb_run(K, c, d):
    """The three kernels through K.lib on guarded buffers: y, y_clamp (gs_embedding_fwd with indices -1 and rows), y_onehot, idx_out (the one-hot
    form), gw, gw_onehot (the backward on idx and on idx_out)."""
    act = np.float32 if c.dtype == F32 else np.uint16
    b, rows, units = c.b, c.rows, c.units
    ins = {k: guarded(d[k]) for k in ("w", "idx", "clamp_idx", "lab", "gy")}
    outs = {"y": poisoned((b, units), act), "y_clamp": poisoned((b, units), act), "y_onehot": poisoned((b, units), act), "idx_out": poisoned((b,), np.int64),
            "gw": poisoned((rows, units), np.float32), "gw_onehot": poisoned((rows, units), np.float32)}
    lib, a, st = K.lib, float(EMB_ALPHA), _stream()
    rcs = [lib.gs_embedding_fwd(ptr(ins["idx"]), ptr(ins["w"]), ptr(outs["y"]), b, rows, units, a, c.dtype, st),
           lib.gs_embedding_fwd(ptr(ins["clamp_idx"]), ptr(ins["w"]), ptr(outs["y_clamp"]), b, rows, units, a, c.dtype, st),
           lib.gs_embedding_onehot_fwd(ptr(ins["lab"]), ptr(ins["w"]), ptr(outs["y_onehot"]), ptr(outs["idx_out"]), b, rows, units, a, c.dtype, st),
           lib.gs_embedding_bwd(ptr(ins["idx"]), ptr(ins["gy"]), ptr(outs["gw"]), b, rows, units, a, c.dtype, st),
           lib.gs_embedding_bwd(ptr(outs["idx_out"]), ptr(ins["gy"]), ptr(outs["gw_onehot"]), b, rows, units, a, c.dtype, st)]
    assert rcs == [0] * 5, (rcs, lib.gs_last_error())
    torch.cuda.synchronize()
    assert all(guards_intact(x) for x in list(ins.values()) + list(outs.values())), ("guard words", emb_id(c))
    for k in ins:
        assert same_bits(payload(ins[k], d[k].dtype, d[k].shape), d[k]), ("input changed", emb_id(c), k)
    shapes = {"idx_out": (b,), "gw": (rows, units), "gw_onehot": (rows, units)}
    return {k: payload(x, np.int64 if k == "idx_out" else (np.float32 if k.startswith("gw") else act), shapes.get(k, (b, units))) for k, x in outs.items()}


# ========================================================================================================================= weight prep
PREP_FWD, PREP_BWD_DATA, PREP_T_FWD, PREP_T_BWD_DATA = 0, 1, 2, 3   # GS_PREP_*
PREP_NAMES = ("fwd", "bwd_data", "t_fwd", "t_bwd_data")
PrepCase = namedtuple("PrepCase", "map ci co ksize stride dtype")
PREP_BLOCKS = 48   # blocks per descriptor of the launch


def _prep_cases():
    out = []
    for dt in DTYPES:
        out += [PrepCase(PREP_FWD, 32, 32, 3, 1, dt), PrepCase(PREP_FWD, 96, 40, 3, 1, dt), PrepCase(PREP_FWD, 96, 160, 3, 2, dt), PrepCase(PREP_FWD, 5, 7, 3, 1, dt),
                PrepCase(PREP_FWD, 1, 16, 3, 1, dt), PrepCase(PREP_FWD, 32, 2, 1, 1, dt), PrepCase(PREP_FWD, 2, 32, 1, 1, dt),
                PrepCase(PREP_BWD_DATA, 32, 2, 1, 1, dt), PrepCase(PREP_BWD_DATA, 2, 32, 1, 1, dt),
                PrepCase(PREP_BWD_DATA, 32, 32, 3, 1, dt), PrepCase(PREP_BWD_DATA, 32, 32, 3, 2, dt), PrepCase(PREP_BWD_DATA, 96, 40, 3, 1, dt),
                PrepCase(PREP_BWD_DATA, 160, 96, 3, 2, dt), PrepCase(PREP_BWD_DATA, 5, 7, 3, 1, dt), PrepCase(PREP_BWD_DATA, 7, 5, 3, 2, dt),
                PrepCase(PREP_T_FWD, 64, 32, 3, 2, dt), PrepCase(PREP_T_BWD_DATA, 64, 32, 3, 2, dt)]
    out += [PrepCase(PREP_FWD, 256, 256, 3, 1, BF16),                                               # 144 tiles on 48 blocks: three trips
            PrepCase(PREP_FWD, 16, 32, 3, 1, F32), PrepCase(PREP_BWD_DATA, 16, 32, 3, 1, F32)]     # fp32: the forward is MFMA-eligible, the data gradient is not
    return out


PREP_CASES = _prep_cases()


def prep_id(c):
    return f"prep-{PREP_NAMES[c.map]}-{DTYPE_NAMES[c.dtype]} {c.ksize}x{c.ksize} {c.ci}->{c.co} s{c.stride}"


def igemm_supported(ic, oc, dtype):
    return ic % (16 if dtype == F32 else 32) == 0 and oc % 32 == 0


def prep_plan(c):
    """(variant, stored as fp32) -- csrc/conv_api.hip: prep_plan and the stride-2 line of the kernel, restated."""
    fwd = c.map in (PREP_FWD, PREP_T_FWD)
    variant = 0 if fwd else (1 if c.map == PREP_BWD_DATA and c.stride != 2 else 2)
    mfma = (c.ksize == 3 or c.map == PREP_T_BWD_DATA) and (igemm_supported(c.ci, c.co, c.dtype) if fwd else igemm_supported(c.co, c.ci, c.dtype))
    return variant, (not mfma) or c.dtype == F32


def prep_facts(c):
    variant, f32 = prep_plan(c)
    taps = c.ksize * c.ksize
    tiles = taps * -(-c.ci // 64) * -(-c.co // 64)
    return {"variant": variant, "f32": f32, "tiles": tiles, "trips": -(-tiles // PREP_BLOCKS), "partial_ci": c.ci % 64 != 0, "partial_co": c.co % 64 != 0,
            "scalar_read": c.co % 4 != 0, "scalar_write": (c.ci if variant == 0 else c.co) % 4 != 0}


def prep_weight(c):
    rng = np.random.default_rng(4000 + 13 * c.ci + c.co + c.map)
    return rng.standard_normal((c.ksize, c.ksize, c.ci, c.co)).astype(np.float32)


def prep_expected(c, w):
    """The operand's bytes: [tap][co][ci] (the transpose) for a forward map, [taps - 1 - tap][ci][co] for the stride-1 data gradient, a copy else."""
    variant, f32 = prep_plan(c)
    w3 = w.reshape(c.ksize * c.ksize, c.ci, c.co)
    op = np.ascontiguousarray(np.transpose(w3, (0, 2, 1)) if variant == 0 else (w3[::-1] if variant == 1 else w3))
    return op if f32 else bf16_bits(op)


def prep_table(cases, wbufs, obufs):
    """The device table as kernels.refresh_weights builds it: 40-byte rows, two pointers and six int32."""
    rows = np.zeros((len(cases), 5), dtype=np.int64)
    for i, c in enumerate(cases):
        rows[i, 0], rows[i, 1] = ptr(wbufs[i]), ptr(obufs[i])
        rows[i, 2:5] = np.array([c.map, c.ci, c.co, c.ksize, c.stride, c.dtype], dtype=np.int32).view(np.int64)
    return torch.from_numpy(rows).cuda()


def prep_run(K, cases, weights):
    """ONE launch over all `cases`: the operands' bytes, each read back from its own guarded buffer.  Every buffer has room for the fp32 form
    (what the library's workspace holds), poisoned: the bytes behind a bf16 operand's last byte are the sentinel, and must keep the poison."""
    expected = [prep_expected(c, w) for c, w in zip(cases, weights)]
    wbufs = [guarded(w) for w in weights]
    obufs = [poisoned(w.shape, np.float32) for w in weights]
    table = prep_table(cases, wbufs, obufs)
    rc = K.lib.gs_weight_prep_batch(table.data_ptr(), len(cases), _stream())
    assert rc == 0, (rc, K.lib.gs_last_error())
    torch.cuda.synchronize()
    assert all(guards_intact(b) for b in wbufs + obufs), "guard words"
    out = []
    for c, w, b, e in zip(cases, weights, wbufs, expected):
        assert same_bits(payload(b, np.float32, w.shape), w), ("weight changed", prep_id(c))
    for c, b, e in zip(cases, obufs, expected):
        raw = payload(b, np.uint8)
        assert bool((raw[e.nbytes:] == POISON_BYTE).all()), ("bytes behind the operand", prep_id(c))
        out.append(raw[:e.nbytes].copy().view(e.dtype).reshape(e.shape))
    return out


# the header's promise, through the public entry points: (ksize, ci, co, stride, input h, w)
PROMISE_LAYERS = ((3, 32, 32, 1, 4, 8), (3, 6, 40, 1, 5, 6), (1, 32, 2, 1, 4, 8))


# ============================================================================================================================== run
def loss_forms(c):
    """(kind, form) of every launch of a loss case (the mode-seeking half alone is an fp32 call whatever the activations are)."""
    return [("d", f) for f in D_FORMS] + [("g", f) for f in G_FORMS if f != "ssq" or c.dtype == F32]


def run(K, case, inputs):
    """The kernels of one case: Adam -> {entry: buffers afterwards}; losses -> {(kind, form): results}; embedding -> results; a tuple of prep
    cases (inputs: their weights) -> their operands from ONE launch."""
    if isinstance(case, AdamCase):
        return {e: adam_run(K, case, inputs, e) for e in ADAM_ENTRIES}
    if isinstance(case, LossCase):
        return {kf: loss_run(K, case, inputs, *kf) for kf in loss_forms(case)}
    if isinstance(case, EmbCase):
        return emb_run(K, case, inputs)
    return prep_run(K, list(case), inputs)
