"""GPU: every route of the spectral kernels against float64 (tests/spectral_cover.py: the cases, the references, the tolerances -- the
project's own, from tests/test_spectral_gpu.py).  Each case asserts the route the library takes first, then compares element-wise.  The
measurement knobs are read once per process: each runs the knob case in a fresh interpreter.  The last test prints the worst ratio
(error / tolerance) per family."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import spectral_cover as C

pytestmark = pytest.mark.gpu
WORST = {}            # family -> worst error / tolerance seen by this module
KNOB_TIMEOUT = 45     # seconds: the child's imports (2.3 s measured, torch already in the page cache), one plan, two launches


def _note(family, value):
    WORST[family] = max(WORST.get(family, 0.0), float(value))


@pytest.fixture(scope="module")
def lib():
    from gansynth_amd import kernels
    assert C.knobs_unset(), "the cases name the routes of the default knobs"
    return kernels.get().lib


@pytest.fixture(scope="module")
def plans():
    made = {}

    def get(c, with_inverse=False):
        if (c.name, with_inverse) not in made:
            made[(c.name, with_inverse)] = C.Plan(c, with_inverse)
        return made[(c.name, with_inverse)]
    yield get
    for p in made.values():
        p.close()


def _route(lib, c, ws_bytes=None):
    """The route the library takes for the case: the one the restatement gives, and the one the case names."""
    r = C.case_lib_route(lib, c, ws_bytes)
    assert r == C.case_route(c, ws_bytes), (c.name, r, C.case_route(c, ws_bytes))
    if ws_bytes is None:
        for f, v in c.expect.items():
            assert r[f] == v, (c.name, f, r[f], v)
    return r


def _images(plan, w, dtype=C.F32, ws_bytes=None):
    img = C.run_fused(plan, w, dtype, ws_bytes)
    assert torch.isfinite(img.float()).all()
    return img


@pytest.mark.parametrize("name", [c.name for c in C.CASES if c.fwd])
def test_forward_vs_float64(name, lib, plans):
    c = C.BY_NAME[name]
    r = _route(lib, c)
    plan, rows = plans(c), list(C.ref_rows(c))
    assert plan.lib.gs_stft_mel_if_workspace_bytes(plan.handle, c.batch) == r["fwd_workspace_bytes"]
    for dtype in c.fwd:
        img = _images(plan, C.waves(c), dtype)[rows].float().cpu().numpy()
        out = C.compare_forward(c, img[..., 0], img[..., 1], dtype)
        tag = ("wave" if r["fwd_kind"] == C.FWD_WAVE else "generic") + (" bf16" if dtype == C.BF16 else "")
        for fam in ("mel", "log", "IF", "pad"):
            _note(f"forward {tag}: {fam}", out[fam])
        print(f"{name} {tag}: " + ", ".join(f"{k} {v:.3g}" for k, v in out.items()))


@pytest.mark.parametrize("name,alone", [("w8_b5", None), ("w16_b300", None), ("w16_b257", (0, 128, 256)), ("w32_b200", (0, 101, 199))])
def test_rows_do_not_depend_on_the_batch(name, alone, lib, plans):
    """Row i of the batch == the same row computed alone, to the bit: blocks that span examples (runs < 12, no exchange, a partial last block)
    against the one-example launch (runs = 12 or 8, exchange where it applies)."""
    c = C.BY_NAME[name]
    _route(lib, c)
    plan, w = plans(c), C.waves(c)
    img = _images(plan, w)
    for i in (range(c.batch) if alone is None else alone):
        assert torch.equal(C.run_fused(plan, w[i:i + 1])[0], img[i]), (name, i)
    if name == "w8_b5":   # the same route alone (eight runs): a two-example launch against it as well
        assert torch.equal(C.run_fused(plan, w[3:5]), img[3:5])


def test_recompute_route_equals_exchange_route(lib, plans):
    """gs_stft_mel_if_fwd with a workspace of 0 bytes: every run recomputes its lead frame; the images equal the exchange route's to the bit."""
    c = C.BY_NAME["w32_b3"]
    assert _route(lib, c)["exchange"] == 1 and _route(lib, c, ws_bytes=0)["exchange"] == 0
    plan = plans(c)
    for dtype in c.fwd:
        assert torch.equal(_images(plan, C.waves(c), dtype, ws_bytes=0), _images(plan, C.waves(c), dtype)), dtype


@pytest.mark.parametrize("name", C.STAGEWISE)
def test_stagewise_vs_float64(name, lib, plans):
    """gs_stft_fwd on both forward paths; on the caller-supplied matrices gs_mel_project and gs_if_unwrap too, each on the oracle's own
    intermediates (float32), against float64 arithmetic on those."""
    c = C.BY_NAME[name]
    _route(lib, c)
    plan = plans(c)
    st64 = C.forward_reference(c)[0]
    mag, ph = C.run_stft(plan, C.waves(c))
    scale = st64["magnitude"].max(axis=(1, 2), keepdims=True)
    _note("stage-wise: magnitude", (np.abs(mag - st64["magnitude"]) / (C.TOL_MAG * scale)).max())
    strong = st64["magnitude"] > C.LOUD * scale                  # phase is only defined where there is signal
    _note("stage-wise: phase", np.abs(np.angle(np.exp(1j * (ph - st64["phase"]))))[strong].max() / 1e-3)
    pads = C.padding_frames(c)
    assert np.all(mag[:, pads] == 0) and np.all(ph[:, pads] == 0)
    assert WORST["stage-wise: magnitude"] < 1.0 and WORST["stage-wise: phase"] < 1.0, WORST
    if c.mel:
        mel64 = C.linear_mel64(c)
        mag32 = st64["magnitude"].astype(np.float32)
        want = mag32.astype(np.float64) @ mel64
        _note("stage-wise: mel_project", np.abs(C.run_mel_project(plan, mag32) - want).max() / (1e-5 * want.max()))
        ph32 = st64["mel_phase"].astype(np.float32)
        want_if = C.S.instantaneous_frequency(ph32.astype(np.float64), axis=-2)
        _note("stage-wise: if_unwrap", np.abs(C.run_if_unwrap(plan, ph32) - want_if).max() / 1e-5)   # same inputs, same recurrence: no modulo
        assert WORST["stage-wise: mel_project"] <= 1.0 and WORST["stage-wise: if_unwrap"] < 1.0, WORST


@pytest.mark.parametrize("name", [c.name for c in C.CASES if c.inv])
def test_inverse_vs_float64(name, lib, plans):
    c = C.BY_NAME[name]
    r = _route(lib, c)
    plan = plans(c, with_inverse=True)
    for dtype in c.inv:
        lm, mi = C.inverse_inputs(c, dtype)           # bf16: the reference starts from the widened bf16 values
        got = C.run_inverse(plan, lm, mi, dtype)
        assert got.shape == (c.batch, c.wave_len) and np.isfinite(got).all()
        worst, corr = C.compare_inverse(got, C.inverse_reference(c, lm, mi))
        tag = {C.ISTFT_WAVE_OLA: "wave + OLA", C.ISTFT_WAVE_FRAMES: "wave, OLA kernel", C.ISTFT_BLOCK_FFT: "block FFT"}[r["istft_kind"]]
        _note(f"inverse {tag}" + (" bf16" if dtype == C.BF16 else ""), worst)
        print(f"{name} {'bf16' if dtype == C.BF16 else 'fp32'}: {worst:.3g} of the tolerance, correlation 1 - {1 - corr:.2e}")


def test_inverse_rows_do_not_depend_on_the_batch(lib, plans):
    c = C.BY_NAME["i40_b2"]
    plan = plans(c, with_inverse=True)
    lm, mi = C.inverse_inputs(c)
    both = C.run_inverse(plan, lm, mi)
    assert np.array_equal(C.run_inverse(plan, lm[1:], mi[1:])[0], both[1])


@pytest.fixture(scope="module")
def knob_inputs(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("spectral_knobs") / "case.npz")
    C.save_knob_inputs(path)
    return path


@pytest.mark.parametrize("env_name,value,knob", C.KNOB_SETTINGS, ids=C.KNOB_NAMES)
def test_knob_routes(env_name, value, knob, knob_inputs):
    """One knob, one fresh interpreter: the route the library reports there is the restatement's under that knob, and the result meets the
    same float64 reference.  A child that dies on a signal or runs into the time limit fails the test, once."""
    c = C.BY_NAME[C.KNOB_CASE]
    env = {k: v for k, v in os.environ.items() if k not in C.KNOB_NAMES}
    env["PYTHONPATH"] = C.ROOT + os.pathsep + env.get("PYTHONPATH", "")
    env[env_name] = value
    try:
        res = subprocess.run([sys.executable, os.path.join(C.ROOT, "tests", "spectral_cover.py"), knob_inputs], env=env, capture_output=True, text=True,
                             timeout=KNOB_TIMEOUT)
    except subprocess.TimeoutExpired as e:
        pytest.fail(f"{env_name}: the child did not finish in {KNOB_TIMEOUT} s: {str(e.stderr)[-1500:]}")
    assert res.returncode >= 0, f"{env_name}: the child died on signal {-res.returncode}: {res.stderr[-1500:]}"
    assert res.returncode == 0, (env_name, res.stdout[-1500:], res.stderr[-3000:])
    out = json.loads(res.stdout.strip().splitlines()[-1])
    want = C.case_route(c, k=C.knobs(**knob))
    got = {f: (tuple(v) if isinstance(v, list) else v) for f, v in out["route"].items()}
    assert got == want and want != C.case_route(c), (env_name, got, want)
    assert out["inverse"] < 1.0 and out["corr"] > C.MIN_CORR, out
    _note(f"knob {env_name}: inverse", out["inverse"])
    if env_name == "GS_SPECTRAL_GENERIC":
        assert want["fwd_kind"] == C.FWD_GENERIC and want["istft_kind"] == C.ISTFT_BLOCK_FFT
        fwd = out["forward"]
        assert fwd["mel"] < 1.0 and fwd["log"] < 1.0 and fwd["IF"] < 1.0 and fwd["pad"] <= 1.0, fwd
        for fam in ("mel", "log", "IF"):
            _note(f"knob {env_name}: forward {fam}", fwd[fam])
    print(f"{env_name}: {out}")


def test_report_worst_ratios():
    """(last in the file) the worst error / tolerance per family over the cases above."""
    assert WORST and all(v <= 1.0 for v in WORST.values()), WORST
    for k in sorted(WORST):
        print(f"  {k:44s} {WORST[k]:.3g}")
