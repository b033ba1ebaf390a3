"""GPU: the kernels that run every iteration outside the route-driven covers -- the four instantiations of adam_tf_kernel (csrc/elementwise.hip), the
two GAN losses and the three embedding kernels (csrc/small_ops.hip) in fp32 and bf16, and weight_prep_batch_kernel (csrc/conv_api.hip) -- against
float64 on the operands as stored, element by element, under the bounds tests/step_cover.py derives by counting roundings (its docstring; the CPU
file holds an fp32 restatement of every kernel's arithmetic against the same bounds).

One test per kernel and dtype.  Every comparison prints `STEP-COVER <case> <result> ratio ...` (worst |error| / bound of that result) before it
asserts: run with -s.  Every buffer a kernel writes sits between guard bytes that are checked after the call, every buffer it only reads is compared
bit for bit afterwards.  The library reads GS_EW_GRID_CAP once per process: the Adam cases run a second time with it set to 2 -- two blocks, 32 trips
of the grid-stride loop at 64003 elements -- in ONE child process, started once under a time limit by the first test that needs it and never again.

Adam: 12 sizes x 3 (beta1, beta2) x 2 grad scales through the by-value entry, the zero-grad entry and the device-scalar entry with zero_grad 0 and
1; from 255 elements on with an all-zero run (which stays +0.0 in all four buffers), runs with g = 0, with v = 0, with b1 m and (1 - b1) g gs
cancelling, with denormal v and with |g| up to 1e15; g untouched bit for bit without ZERO and +0.0 everywhere with it; the device-scalar entry
gives the bits of the by-value entry, and a negative scalar leaves everything untouched.  Losses: 8 shapes, every pinned logit, all seven forms,
the gradients of a half alone bit-equal to those of the whole.  Embedding: 6 shapes, the clamp, five kinds of label rows.  Weight prep: 37
descriptors in one launch and each alone, byte for byte, and the promise of include/gansynth_hip.h through conv2d_fwd / conv2d_bwd_data.

Worst ratios (|error| / bound, so 1 is the bound) measured on the MI355X, knob unset / set to 2 -- records, not bounds:
  adam_tf_kernel, all four instantiations alike (the device-scalar entry gives the by-value entry's bits): m' 0.23 / 0.23, v' 0.16 / 0.16, p' 0.49 / 0.49
  (864 + 864 comparisons).  The rest has no knob: gan_d_loss fp32 loss 0.028, g_real 0.053, g_fake 0.058, g_penalty 0.20; bf16 loss 0.034, g_real and
  g_fake 0.97 (the one rounding of the store, 2^-8 |ref|, is the bound), g_penalty 0.20; gan_g_loss fp32 loss 0.029, g_fake 0.064, g_sumsq 0.26; bf16
  loss 0.024, g_fake 0.96, g_sumsq 0.26; embedding_bwd fp32 0.55, bf16 gy 0.65 (a row with one sample has one rounding against a bound of one u);
  embedding_fwd, embedding_onehot_fwd, the 37 prepared operands (together and alone) and the 12 conv results behind a refresh: exact.
The first run of this file found no wrong element in any of these kernels.  What it does hold, from a scratch build with one value changed at a
time (no address touched), this file against tests/test_kernels_gpu.py as it stood: `b1 * mm[e]` -> `0.f` in the vector loop of adam_tf_kernel
fails here, passes there; `if (ZERO) g[t] = 0.f` removed from the tail fails here and in test_adam_tf_step_with_lr_from_device_memory[True] there (its
100003 elements have a tail: that one was held already); `k += 128` in gan_d_loss_kernel, `v >= best` in the one-hot scan and `tt = t` in variant 1 of
the prep kernel fail here and pass there.
"""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tests import step_cover as C  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def K():
    from gansynth_amd import kernels
    assert not set(C.KNOBS) & set(os.environ), "the parent process runs with the knob unset"
    return kernels.HipKernels()


def _report(case, ratios, bad):
    for name in sorted(ratios):
        print(f"STEP-COVER {case} {name} ratio {ratios[name]:.3e}")
    assert not bad, (case, bad, ratios)


# ------------------------------------------------------------------------------------------------------------------------------ Adam
@functools.lru_cache(maxsize=None)
def _adam_case(c):
    d = C.adam_inputs(c)
    return d, C.adam_reference(c, d)


def check_adam(K, c, entries=C.ADAM_ENTRIES):
    """One case through `entries`; returns {entry: {result: ratio}}."""
    d, ref = _adam_case(c)
    got = {e: C.adam_run(K, c, d, e) for e in entries}
    out = {}
    for e in entries:
        ratios, bad = C.adam_check(c, d, got[e], e, ref)
        for dev, val in (("dev", "value"), ("dev_zero", "zero")):   # the same fp32 lr_t from device memory: the same bits
            if e == dev and val in got and not all(C.same_bits(got[dev][k], got[val][k]) for k in "pgmv"):
                bad.append(f"{dev} differs from {val}")
        _report(f"{C.adam_id(c)} {e}", ratios, bad)
        out[e] = ratios
    return out


class _KnobChild(object):
    """Every Adam case once more with the knob set, in one child process started when the first test asks; a time limit, no second try."""
    def __init__(self):
        self.results, self.failed = None, None

    def get(self, c):
        if self.results is None and self.failed is None:
            self.failed = ("not finished", "", "")   # (marked before the spawn: whatever happens below, the child is started once)
            env = dict(os.environ, **C.KNOBS)
            env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
            try:
                r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=300)
            except subprocess.TimeoutExpired as e:
                self.failed = ("the time limit", str(e.stdout)[-1500:], str(e.stderr)[-3000:])
            else:
                print(r.stdout[-400000:])
                try:
                    assert r.returncode == 0
                    self.results, self.failed = json.loads(r.stdout.strip().splitlines()[-1]), None
                except (AssertionError, ValueError, IndexError):
                    self.failed = (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
        assert self.failed is None, f"the knob child ended with {self.failed[0]}; it is not started again: {self.failed[1:]}"
        return self.results[C.adam_id(c)]


@pytest.fixture(scope="module")
def knob_child():
    return _KnobChild()


@pytest.mark.parametrize("pair", (("value", "dev"), ("zero", "dev_zero")), ids=("adam_tf_kernel-keep_g", "adam_tf_kernel-zero_g"))
def test_adam_matches_float64(K, knob_child, pair):
    """adam_tf_kernel<ZERO, false> and <ZERO, true> of one ZERO: the by-value entry and the device-scalar entry on the same operands."""
    for c in C.ADAM_CASES:
        check_adam(K, c, pair)
    for c in C.ADAM_CASES:
        res = knob_child.get(c)
        assert res["ok"], (C.adam_id(c), res["error"])


def test_adam_negative_device_scalar_leaves_every_buffer_untouched(K):
    for n in C.ADAM_SKIP_SIZES:
        c = C.AdamCase(n, 0.9, 0.999, 0.5)
        d, _ = _adam_case(c)
        for e in ("dev", "dev_zero"):
            got = C.adam_run(K, c, d, e, lr_t=np.float32(-1.0))
            assert all(C.same_bits(got[k], d[k]) for k in "pgmv"), (n, e)


# ---------------------------------------------------------------------------------------------------------------------------- losses
_LOSS = {}


def check_loss(K, c, kind):
    if c not in _LOSS:   # the seven launches of a case, once for the two tests that read them
        d = C.loss_inputs(c)
        _LOSS[c] = (d, C.run(K, c, d))
    d, results = _LOSS[c]
    got = {form: r for (k, form), r in results.items() if k == kind}
    for form in got:
        ratios, bad = C.loss_check(c, d, got[form], C.loss_reference(c, d, kind, form))
        _report(f"{C.loss_id(c)} {kind}:{form}", ratios, bad)
    if kind == "d":   # either half alone, with or without the penalty: the same numbers
        same = [("both", "both+pen", "g_real"), ("both", "both+pen", "g_fake"), ("both", "real", "g_real"), ("both", "fake", "g_fake")]
    else:
        same = [("fake", "fake+ssq", "g_fake")] + ([("ssq", "fake+ssq", "g_ssq")] if "ssq" in got else [])
    for a, b, name in same:
        assert C.same_bits(got[a][name], got[b][name]), (C.loss_id(c), kind, a, b, name)


@pytest.mark.parametrize("dtype", C.DTYPES, ids=C.DTYPE_NAMES)
def test_gan_d_loss_matches_float64(K, dtype):
    for c in C.LOSS_CASES:
        if c.dtype == dtype:
            check_loss(K, c, "d")


@pytest.mark.parametrize("dtype", C.DTYPES, ids=C.DTYPE_NAMES)
def test_gan_g_loss_matches_float64(K, dtype):
    for c in C.LOSS_CASES:
        if c.dtype == dtype:
            check_loss(K, c, "g")


# ------------------------------------------------------------------------------------------------------------------------- embedding
_EMB = {}


def _emb(K, c):
    """The five launches of a case, once for the three tests that read them."""
    if c not in _EMB:
        d = C.emb_inputs(c)
        _EMB[c] = (d, C.run(K, c, d))
    return _EMB[c]


@pytest.mark.parametrize("dtype", C.DTYPES, ids=C.DTYPE_NAMES)
def test_embedding_fwd_is_the_rounded_product(K, dtype):
    for c in (x for x in C.EMB_CASES if x.dtype == dtype):
        d, got = _emb(K, c)
        ok = C.same_bits(got["y"], C.emb_forward_bits(c, d["w"], d["idx"]))
        clamp = C.same_bits(got["y_clamp"], C.emb_forward_bits(c, d["w"], d["clamp_idx"]))   # -1 reads row 0, rows reads row rows - 1
        print(f"STEP-COVER {C.emb_id(c)} y exact {int(ok)} y_clamp exact {int(clamp)} ratio {0.0 if ok and clamp else float('inf'):.3e}")
        assert ok and clamp, C.emb_id(c)


@pytest.mark.parametrize("dtype", C.DTYPES, ids=C.DTYPE_NAMES)
def test_embedding_onehot_fwd_takes_the_first_maximum(K, dtype):
    for c in (x for x in C.EMB_CASES if x.dtype == dtype):
        d, got = _emb(K, c)
        want = C.first_max(d["lab"])
        ok_idx = np.array_equal(got["idx_out"], want)
        ok_y = C.same_bits(got["y_onehot"], C.emb_forward_bits(c, d["w"], want))
        print(f"STEP-COVER {C.emb_id(c)} idx_out exact {int(ok_idx)} y_onehot exact {int(ok_y)} ratio {0.0 if ok_idx and ok_y else float('inf'):.3e}")
        assert ok_idx and ok_y, (C.emb_id(c), got["idx_out"].tolist(), want.tolist())


@pytest.mark.parametrize("dtype", C.DTYPES, ids=C.DTYPE_NAMES)
def test_embedding_bwd_matches_float64(K, dtype):
    for c in (x for x in C.EMB_CASES if x.dtype == dtype):
        d, got = _emb(K, c)
        for name, idx in (("gw", d["idx"]), ("gw_onehot", C.first_max(d["lab"]))):
            ref, bound, unselected = C.emb_backward_reference(c, d, idx)
            err = np.abs(got[name].astype(np.float64) - ref)
            ratio = float(np.max(np.where(err == 0, 0.0, err / np.maximum(bound, 1e-300))))
            bad = [] if bool((err <= bound).all()) else [name]
            if not C.same_bits(got[name][unselected], np.zeros((len(unselected), c.units), dtype=np.float32)):
                bad.append(name + ": a row no sample selects is not +0.0")
            _report(f"{C.emb_id(c)}", {name: ratio}, bad)


# ----------------------------------------------------------------------------------------------------------------------- weight prep
def test_weight_prep_batch_writes_the_operands_byte_for_byte(K):
    cases = C.PREP_CASES
    weights = [C.prep_weight(c) for c in cases]
    expected = [C.prep_expected(c, w) for c, w in zip(cases, weights)]
    together = C.run(K, tuple(cases), weights)   # one table, one launch: blockIdx.y over all descriptors
    bad = []
    for c, w, e, g in zip(cases, weights, expected, together):
        alone = C.run(K, (c,), [w])[0]
        ok, ok_alone = C.same_bits(g, e), C.same_bits(alone, e)
        wrong = int((g != e).sum()) if g.shape == e.shape else -1
        print(f"STEP-COVER {C.prep_id(c)} operand exact {int(ok)} alone exact {int(ok_alone)} wrong elements {wrong} ratio {0.0 if ok and ok_alone else float('inf'):.3e}")
        if not (ok and ok_alone):
            bad.append(C.prep_id(c))
    assert not bad, bad


@pytest.mark.parametrize("dtype", C.DTYPES, ids=C.DTYPE_NAMES)
def test_refreshed_operands_serve_the_convs_like_their_own(dtype):
    """include/gansynth_hip.h: gs_weight_prep_batch "writes exactly what the map's entry point would write with w_prepared = 0".  Weights of a
    registered buffer, changed and refreshed in one launch, then read by conv2d_fwd / conv2d_bwd_data with w_prepared = 1, against the same calls
    on unregistered clones (a transient workspace, w_prepared = 0): the same bits."""
    from gansynth_amd import kernels
    K = kernels.HipKernels()
    tdt = (torch.float32, torch.bfloat16)[dtype]
    gen = torch.Generator().manual_seed(11)
    sizes = [k * k * ci * co for k, ci, co, *_ in C.PROMISE_LAYERS]
    starts = np.cumsum([0] + [-(-s // 64) * 64 for s in sizes])
    flat = torch.randn(int(starts[-1]), generator=gen).cuda()
    K.register_param_buffer(flat)
    ws = [flat[int(a):int(a) + s].view(k, k, ci, co) for a, s, (k, ci, co, *_) in zip(starts, sizes, C.PROMISE_LAYERS)]
    flags = []
    inner = K._weight_ws

    def spy(*a, **kw):
        r = inner(*a, **kw)
        flags.append(r[1])
        return r
    K._weight_ws = spy

    def layer_io(i):
        k, ci, co, stride, h, wd = C.PROMISE_LAYERS[i]
        x = torch.randn(2, ci, h, wd, generator=gen).to(tdt).cuda().contiguous(memory_format=torch.channels_last)
        gy = torch.randn(2, co, h // stride, wd // stride, generator=gen).to(tdt).cuda().contiguous(memory_format=torch.channels_last)
        return x, gy

    def both_maps(w, i, x, gy):
        k, ci, co, stride, h, wd = C.PROMISE_LAYERS[i]
        return K.conv2d_fwd(x, w, k, stride, 0.5), K.conv2d_bwd_data(gy, w, tuple(x.shape), k, stride, 0.5)
    io = [layer_io(i) for i in range(len(ws))]
    for i, w in enumerate(ws):   # the first calls create the persistent workspaces (and lay out the OLD values)
        both_maps(w, i, *io[i])
    assert flags == [0] * (2 * len(ws))
    flat.copy_(torch.randn(flat.numel(), generator=gen).cuda())
    K.invalidate_weights(flat)
    assert K.refresh_weights(flat) == 2 * len(ws)   # every (weight, map) operand, one launch
    del flags[:]
    for i, w in enumerate(ws):
        y, gx = both_maps(w, i, *io[i])
        assert flags[-2:] == [1, 1], flags
        y0, gx0 = both_maps(w.clone(), i, *io[i])
        assert flags[-2:] == [0, 0], flags
        torch.cuda.synchronize()
        for name, a, b in (("fwd", y, y0), ("bwd_data", gx, gx0)):
            same = torch.equal(a.view(torch.int32 if dtype == C.F32 else torch.int16), b.view(torch.int32 if dtype == C.F32 else torch.int16))
            print(f"STEP-COVER promise-{C.DTYPE_NAMES[dtype]} {C.PROMISE_LAYERS[i][:3]} {name} exact {int(same)} ratio {0.0 if same else float('inf'):.3e}")
            assert same and bool(torch.isfinite(a.float()).all()), (C.PROMISE_LAYERS[i], name)


def _child():
    """With the knob of this process's environment: every Adam case through the four entries, checked; one JSON line of results.  A failed
    assertion is a result; anything else (a HIP error among them) ends the child with a non-zero status."""
    from gansynth_amd import kernels
    assert os.environ["GS_EW_GRID_CAP"] == C.KNOBS["GS_EW_GRID_CAP"]
    K = kernels.HipKernels()
    out = {}
    for c in C.ADAM_CASES:
        try:
            out[C.adam_id(c)] = {"ok": True, "ratio": check_adam(K, c)}
        except AssertionError as e:
            out[C.adam_id(c)] = {"ok": False, "error": str(e)[-1500:]}
    torch.cuda.synchronize()
    print(json.dumps(out))


if __name__ == "__main__":
    _child()
