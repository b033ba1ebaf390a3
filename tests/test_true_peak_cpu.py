"""CPU: the true-peak rule's float64 restatement (tests/true_peak_ref.py) against analysis and against the condition the limiter is built
for, the library's 1 -> 4 table against the resampler's design, and every host-side check of gs_true_peak / gs_limit_env, the Python layer
and the driver's --true_peak -- no device is touched.  Every figure is printed before it is asserted."""
import argparse
import ctypes

import numpy as np
import pytest

from tests import limiter_ref as LR
from tests import resample_ref as RR
from tests import true_peak_ref as TR


@pytest.mark.parametrize("period,phase,sample_peak", [(4, np.pi / 4, 0.7071), (8, np.pi / 8, 0.9239)], ids=["fs/4 at 45 deg", "fs/8 at 22.5 deg"])
def test_detector_reads_the_crest_the_samples_miss(period, phase, sample_peak):
    """The 4x grid hits the crest of both sines: away from the clip's ends the reference reads the amplitude within 0.01 dB."""
    amplitude = 1.7
    x = TR.sine(period, phase, amplitude).astype(np.float32)
    assert abs(np.abs(x).max() / amplitude - sample_peak) < 1e-4
    e, bound = TR.detector(x)
    inner = e[4 * TR.TAPS:-4 * TR.TAPS]
    err = TR.db(inner.max() / amplitude)
    print(f"period {period}: sample peak {np.abs(x).max() / amplitude:.4f} A, true peak {inner.max() / amplitude:.6f} A ({err:+.6f} dB), largest bound {bound.max():.3g}")
    assert abs(err) <= 0.01
    assert (e >= np.abs(x).max(axis=0)).all()                                        # never below the sample itself
    assert TR.true_peak(np.zeros((2, 100))) == 0.0 and TR.db(0.0) == -np.inf


@pytest.mark.parametrize("name", ["sine", "noise", "square", "bursts"])
def test_limiter_condition(name):
    """c = -1 dBFS, W = 240: the float64 true-peak limiter's output, re-measured by the float64 detector, stands at most 0.05 dB over c; the
    plain rule's stands more than 1.5 dB over it.  (Measured: 0.0001 / 0.0076 / 0.0014 / 0.0056 dB against 3.11 / 1.85 / 2.06 / 2.21 dB.)"""
    x = TR.inputs()[name]
    with_env, plain = TR.limited_true_peak_db(x, 240, True), TR.limited_true_peak_db(x, 240, False)
    print(f"{name}: true peak over the ceiling {with_env:+.4f} dB with the envelope, {plain:+.4f} dB without")
    assert with_env <= 0.05
    assert plain > 1.5
    # the sample-peak promise holds either way
    y = LR.pre(np.atleast_2d(x).astype(np.float32), 1.0)
    env = TR.scaled_envelope(TR.detector(y)[0], 1.0)
    assert (np.abs(TR.limit_f64(y, env, TR.C, 240).out) <= np.float64(TR.C)).all()


def test_the_restatement_without_an_envelope_is_limiter_ref():
    x = LR.draw(LR.T + 1, 2, 64)
    y = LR.pre(x, LR.D)
    for mine, theirs in ((TR.limit_f64(y, None, LR.C, 64), LR.limit_f64(y, LR.C, 64)), (TR.limit_f32(y, None, LR.C, 64), LR.limit_f32(y, LR.C, 64))):
        assert all(np.array_equal(a, b) for a, b in zip(mine, theirs))
    folded = np.abs(x).max(axis=0)                                                   # env = |x|, rows folded: the plain rule again
    assert np.array_equal(TR.limit_f32(y, TR.scaled_envelope(folded, LR.D), LR.C, 64).out, LR.limit_f32(y, LR.C, 64).out)
    assert np.array_equal(TR.quiet(y, None, LR.C, 64), LR.quiet(y, LR.C, 64))


def _design(_lib, lib):
    design = _lib.GsResample()
    assert lib.gs_resample_design(1, 4, ctypes.byref(design)) == 0
    return design


def test_table_is_the_resamplers():
    """The table the library hands out for 1 -> 4 equals resample_ref.table(4, 1, 68) rounded once to fp32, in both layouts."""
    from gansynth_amd import _lib
    lib = _lib.load()
    design = _design(_lib, lib)
    assert (design.up, design.down, design.taps) == (TR.UP, TR.DOWN, TR.TAPS) == (_lib.TRUE_PEAK_OVERSAMPLE, 1, _lib.TRUE_PEAK_TAPS)
    assert RR.design(1, 4) == (4, 1, 68)
    want = TR.table64().astype(np.float32)
    for layout in (0, 1):
        assert lib.gs_resample_table_bytes(ctypes.byref(design), layout) == 4 * 68 * 4     # 68 is a multiple of 4: no row padding
        host = np.full(4 * 68, np.nan, dtype=np.float32)
        assert lib.gs_resample_table(ctypes.byref(design), layout, host.ctypes.data) == 0
        assert np.array_equal(host.reshape(4, 68).view(np.uint32), want.view(np.uint32))
    assert np.array_equal(TR.table32(), want.astype(np.float64))
    gain = want.astype(np.float64).sum(axis=1)
    print(f"phase sums {gain}")
    assert np.abs(gain - 1).max() < 1e-3 and want[0, 33] < 1.0                              # phase 0 is not the identity


def test_header_constants():
    import os
    import re
    from gansynth_amd import _lib, true_peak
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gansynth_hip.h")).read()
    got = {k: int(v) for k, v in re.findall(r"#define GS_TRUE_PEAK_(TILE|TAPS|OVERSAMPLE) (\d+)", hdr)}
    assert got == dict(TILE=_lib.TRUE_PEAK_TILE, TAPS=_lib.TRUE_PEAK_TAPS, OVERSAMPLE=_lib.TRUE_PEAK_OVERSAMPLE) == dict(TILE=TR.TILE, TAPS=68, OVERSAMPLE=4)
    assert true_peak.OVERSAMPLE == 4


def test_workspace_arithmetic():
    from gansynth_amd import _lib
    lib = _lib.load()
    T = _lib.TRUE_PEAK_TILE
    for n, tiles in ((1, 1), (T, 1), (T + 1, 2), (4 * T, 4), (4 * T + 1, 5), (2880000, 1407), (1 << 40, (1 << 40) // T)):
        for rows in (1, 2):
            assert lib.gs_true_peak_workspace_bytes(rows, n) == (4 * tiles + 15) // 16 * 16, (rows, n)
    for rows, n in ((0, 100), (3, 100), (-1, 100), (1, 0), (2, -5), (1, (1 << 40) + 1)):
        assert lib.gs_true_peak_workspace_bytes(rows, n) == 0, (rows, n)


def test_true_peak_refusals():
    """Dummy pointers: the argument checks come first, nothing is dereferenced or launched."""
    from gansynth_amd import _lib
    lib = _lib.load()
    P, n = 0x10000, 5000
    ws = int(lib.gs_true_peak_workspace_bytes(2, n))
    good = dict(table=P, x=P, rows=2, n=n, stride=n, env=P, peak=P, ws=P, ws_bytes=ws)

    def call(**change):
        a = dict(good, **change)
        return lib.gs_true_peak(a["table"], a["x"], a["rows"], a["n"], a["stride"], a["env"], a["peak"], a["ws"], a["ws_bytes"], None)

    bad = [(dict(rows=0), b"rows must be 1 or 2"), (dict(rows=3), b"rows must be 1 or 2"), (dict(n=0), b"n must be in"), (dict(n=-4), b"n must be in"),
           (dict(n=(1 << 40) + 1, stride=(1 << 40) + 1), b"n must be in"), (dict(stride=n - 1), b"row_stride"), (dict(table=None), b"null pointer"),
           (dict(x=None), b"null pointer"), (dict(env=None, peak=None), b"cannot both"), (dict(table=P + 4), b"misaligned"), (dict(x=P + 2), b"misaligned"),
           (dict(env=P + 1), b"misaligned"), (dict(peak=P + 2), b"misaligned"), (dict(ws=None), b"workspace"), (dict(ws=P + 4), b"workspace"),
           (dict(ws_bytes=ws - 1), b"workspace")]
    for change, message in bad:
        assert call(**change) == -1, change
        assert message in lib.gs_last_error() and b"true_peak" in lib.gs_last_error(), (change, lib.gs_last_error())


def test_limit_env_refusals():
    from gansynth_amd import _lib
    lib = _lib.load()
    P, Q, n = 0x10000, 0x80000, 5000
    ws = int(lib.gs_limit_workspace_bytes(2, n))
    good = dict(x=P, env=P, rows=2, n=n, stride=n, d=1.5, c=0.9, W=240, out=Q, out_stride=n, pcm=None, peak=None, gain=None, ws=P, ws_bytes=ws)

    def call(**change):
        a = dict(good, **change)
        return lib.gs_limit_env(a["x"], a["env"], a["rows"], a["n"], a["stride"], a["d"], a["c"], a["W"], a["out"], a["out_stride"], a["pcm"], a["peak"],
                                a["gain"], a["ws"], a["ws_bytes"], None)

    bad = [(dict(env=None), b"env is required"), (dict(env=P + 2), b"env is required"), (dict(rows=3), b"rows must be 1 or 2"), (dict(n=0), b"n must be in"),
           (dict(stride=n - 1), b"row_stride"), (dict(out_stride=n - 1), b"out_stride"), (dict(x=None), b"null pointer"), (dict(out=None), b"null pointer"),
           (dict(x=P + 2), b"misaligned"), (dict(pcm=P + 1), b"misaligned"), (dict(ws_bytes=ws - 1), b"workspace"), (dict(d=0.0), b"pre_gain"),
           (dict(d=float("inf")), b"pre_gain"), (dict(c=1.5), b"ceiling"), (dict(W=0), b"lookahead"), (dict(W=2049), b"lookahead"), (dict(out=P + 16), b"overlap")]
    for change, message in bad:
        assert call(**change) == -1, change
        assert message in lib.gs_last_error(), (change, lib.gs_last_error())
    # gs_limit itself is as it was: no envelope, the same refusals
    assert lib.gs_limit(P, 2, n, n - 1, 1.5, 0.9, 240, Q, n, None, None, None, P, ws, None) == -1 and b"row_stride" in lib.gs_last_error()


def test_python_layer_refusals_need_no_device():
    import torch
    from gansynth_amd import kernels, limiter, loudness, true_peak
    x = torch.zeros(2, 100)
    with pytest.raises(ValueError, match="true_peak: x must be a non-empty fp32"):
        kernels.true_peak(torch.zeros(2, 100, dtype=torch.float64))
    with pytest.raises(ValueError, match="true_peak: x must have 1 or 2 rows"):
        kernels.true_peak(torch.zeros(3, 100))
    with pytest.raises(ValueError, match="true_peak.measure: clip must be"):
        true_peak.measure(torch.zeros(1, 100))
    with pytest.raises(ValueError, match="envelope must be an fp32 vector of the clip's 100 samples"):
        kernels.limit(x, 1.0, 0.9, 8, envelope=torch.zeros(99))
    with pytest.raises(ValueError, match="envelope must be an fp32 vector"):
        kernels.limit(x, 1.0, 0.9, 8, envelope=torch.zeros(100, dtype=torch.float64))
    with pytest.raises(ValueError, match="limiter.apply: clip must be"):
        limiter.apply(torch.zeros(3, 100), 48000, true_peak=True)
    with pytest.raises(ValueError, match="loudness.apply: clip must be"):
        loudness.apply(torch.zeros(3, 100), 48000, -16.0, true_peak=True)
    assert true_peak.to_db(0.0) == -np.inf and abs(true_peak.to_db(0.5) + 6.0206) < 1e-4


def test_design_numbers_with_a_true_peak():
    """limiter.design takes the true peak as the clip's peak: drive_db above the ceiling, and with drive 0 the scaled TRUE peak -- hence every
    fl(d * env[t]) and every |fl(d * x)| under it -- does not round past the fp32 ceiling, so the gain is 1 throughout."""
    from gansynth_amd import limiter
    x = TR.inputs()["sine"].astype(np.float32)
    env = TR.detector(x)[0].astype(np.float32)
    tp = float(env.max())
    assert 1.99 < tp < 2.05 and np.abs(x).max() < 1.4143       # (2.024: the clip starts and stops abruptly, and the band-limited step overshoots)
    d, c, w = limiter.design(48000, -1.0, 6.0, 0.005, tp)
    assert w == 240 and c == 10.0 ** (-1 / 20) and abs(d * tp / c - 10.0 ** (6 / 20)) < 1e-12
    d0, c0, _ = limiter.design(48000, -1.0, 0.0, 0.005, tp)
    scaled = TR.scaled_envelope(env, d0)
    assert scaled.max() <= np.float32(c0) and (np.abs(LR.pre(x, d0)) <= scaled.max()).all()
    assert abs(d0 * tp / c0 - 1) < 2.0 ** -22
    assert (TR.limit_f32(LR.pre(x, d0), scaled, c0, w).g == 1).all()


def test_driver_refuses_true_peak_alone():
    import gan_synth_main as main
    with pytest.raises(SystemExit, match="--true_peak needs --limit or --loudness"):
        main.check_true_peak_args(main.parser.parse_args(["--synthesize", "score.json", "--true_peak"]))
    with pytest.raises(SystemExit, match="--true_peak needs --limit or --loudness"):
        main.main(main.parser.parse_args(["--true_peak"]))
    assert main.check_true_peak_args(main.parser.parse_args(["--synthesize", "score.json", "--limit", "-1", "--true_peak"])) is True
    assert main.check_true_peak_args(main.parser.parse_args(["--synthesize", "score.json", "--loudness", "-16", "--true_peak"])) is True
    assert main.check_true_peak_args(main.parser.parse_args(["--synthesize", "score.json", "--limit", "-1"])) is False
    assert main.check_true_peak_args(argparse.Namespace(synthesize=None)) is False          # (a namespace from before the flag)
