"""GPU: gs_yin_difference / gs_yin_pick / gs_yin_track against the float64 restatement (tests/yin_ref.py), then pitch.track / note_statistics,
GANSynth.evaluate(f0=True) and the driver's --f0.  Every figure is printed before it is asserted.

The kernel tests call the C entries themselves: the inputs sit inside NaN-filled buffers with row slack (ldx = n + 3), once 16-byte aligned and
once one float off, every output inside a sentinel-filled buffer, and nothing outside the outputs may change.

Bounds (u = 2^-24).  d is a fp32 sum of W non-negative terms, each a rounded square of a rounded difference, in a fixed order: within
(W + 8) u, relative, of its float64 value (yin_ref.dist_bound = kmeans_ref.dist_bound), d(0) an exact 0; the power likewise.  Rules 2-4 run in
float64 on the device as in the restatement: on the device's OWN d the lag is identical and period and aperiodicity agree to 1e-12 (slack for
FMA contraction only), except in a frame where a comparison the restatement makes has its two sides within 1e-12 of each other -- and no frame
of these inputs is such a frame (asserted).  gs_yin_track runs the same device code as the other two: bit-identical."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import yin_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD = 64                                   # elements of sentinel on either side of every buffer
I_SENT, F_SENT, D_SENT = -7777, -12345.5, -54321.25
THRESHOLD = 0.15
# (rows, n, W, L, hop, tau_min): one frame with an exact fit; nothing a multiple of anything; hop 1 and many frames; the production parameters
# with one frame (the last sample's neighbour is read) and with ten; a window far above the lags; the upper limits
SHAPES = [(1, 48, 32, 16, 8, 2), (3, 1000, 100, 37, 33, 8), (5, 2307, 257, 129, 1, 2), (4, 1536, 1024, 512, 256, 8), (2, 4000, 1024, 512, 256, 8),
          (1, 1200, 1024, 1024 - 900, 7, 2), (2, 6000, 4096, 1024, 512, 8)]
IDS = [f"rows{r}-n{n}-W{W}-L{L}-hop{hop}-min{tau_min}" for r, n, W, L, hop, tau_min in SHAPES]


def _lib():
    from gansynth_amd import _lib as L
    return L, L.load()


@functools.lru_cache(maxsize=None)
def _inputs(shape):
    rows, n = shape[:2]
    x = R.harmonic_rows(rows, n, seed=1000 * n + rows)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _reference(shape):
    """(d [rows, F, L], power [rows, F]) in float64, read-only."""
    rows, n, W, L, hop, _ = shape
    parts = [R.difference(row, W, L, hop) for row in _inputs(shape)]
    d, power = np.stack([p[0] for p in parts]), np.stack([p[1] for p in parts])
    d.setflags(write=False)
    power.setflags(write=False)
    return d, power


def _place(a, aligned, slack=3):
    """a [rows, n] inside a NaN-filled device buffer, rows n + slack apart, the first on 16 bytes or one float off: -> (buffer, view, ld)."""
    rows, n = a.shape
    ld = n + slack
    off = PAD + (0 if aligned else 1)
    buf = torch.full((off + rows * ld + PAD,), float("nan"), device="cuda")
    view = buf[off:off + rows * ld].view(rows, ld)[:, :n]
    view.copy_(torch.from_numpy(np.array(a)))
    assert (view.data_ptr() % 16 == 0) == aligned
    return buf, view, ld


def _out(count, sentinel, dtype, aligned=True):
    """`count` elements inside a sentinel-filled buffer: -> (buffer, view).  (float64: 8-byte aligned either way, on 16 bytes or off.)"""
    off = PAD + (0 if aligned else 1)
    buf = torch.full((off + count + PAD,), sentinel, dtype=dtype, device="cuda")
    return buf, buf[off:off + count]


def _intact(buf, view, sentinel):
    host = buf.cpu().numpy()
    off = (view.data_ptr() - buf.data_ptr()) // buf.element_size()
    return bool((host[:off] == sentinel).all() and (host[off + view.numel():] == sentinel).all())


@functools.lru_cache(maxsize=None)
def _run(shape, aligned):
    """The three entries on the shape's input: -> dict of host arrays d, power, lag, period, aper (pick after difference) and t_lag, t_period,
    t_aper, t_power (track).  Checks on the way that nothing around an output changed, that the input is as it was and that a second call
    writes the same bits."""
    from gansynth_amd import kernels
    L_, lib = _lib()
    rows, n, W, L, hop, tau_min = shape
    F = lib.gs_yin_frames(n, W, L, hop)
    assert F == R.frames(n, W, L, hop) >= 1
    xbuf, xv, ldx = _place(_inputs(shape), aligned)
    st = kernels._stream()
    dbuf, d = _out(rows * F * L, F_SENT, torch.float32, aligned)
    pbuf, power = _out(rows * F, F_SENT, torch.float32, aligned)
    L_.check(lib.gs_yin_difference(xv.data_ptr(), ldx, rows, n, W, L, hop, d.data_ptr(), power.data_ptr(), st), "gs_yin_difference")
    torch.cuda.synchronize()
    assert _intact(dbuf, d, F_SENT) and _intact(pbuf, power, F_SENT)
    d2buf, d2 = _out(rows * F * L, F_SENT, torch.float32, aligned)
    p2buf, power2 = _out(rows * F, F_SENT, torch.float32, aligned)
    L_.check(lib.gs_yin_difference(xv.data_ptr(), ldx, rows, n, W, L, hop, d2.data_ptr(), power2.data_ptr(), st), "gs_yin_difference")
    torch.cuda.synchronize()
    assert torch.equal(d2, d) and torch.equal(power2, power)                               # two calls: the same bits

    def outputs():
        return (_out(rows * F, I_SENT, torch.int32, aligned), _out(rows * F, D_SENT, torch.float64, aligned), _out(rows * F, D_SENT, torch.float64, aligned))

    (lbuf, lag), (ebuf, period), (abuf, aper) = outputs()
    L_.check(lib.gs_yin_pick(d.data_ptr(), rows, F, L, tau_min, THRESHOLD, lag.data_ptr(), period.data_ptr(), aper.data_ptr(), st), "gs_yin_pick")
    torch.cuda.synchronize()
    assert _intact(lbuf, lag, I_SENT) and _intact(ebuf, period, D_SENT) and _intact(abuf, aper, D_SENT) and _intact(dbuf, d, F_SENT)
    (tlbuf, t_lag), (tebuf, t_period), (tabuf, t_aper) = outputs()
    tpbuf, t_power = _out(rows * F, F_SENT, torch.float32, aligned)
    L_.check(lib.gs_yin_track(xv.data_ptr(), ldx, rows, n, W, L, hop, tau_min, THRESHOLD, t_lag.data_ptr(), t_period.data_ptr(), t_aper.data_ptr(),
                              t_power.data_ptr(), st), "gs_yin_track")
    torch.cuda.synchronize()
    assert _intact(tlbuf, t_lag, I_SENT) and _intact(tebuf, t_period, D_SENT) and _intact(tabuf, t_aper, D_SENT) and _intact(tpbuf, t_power, F_SENT)
    assert np.isnan(xbuf.cpu().numpy()).sum() == xbuf.numel() - rows * n                   # the input and its surroundings are as they were
    assert np.array_equal(xv.cpu().numpy(), _inputs(shape))
    host = dict(d=d.view(rows, F, L), power=power.view(rows, F), lag=lag.view(rows, F), period=period.view(rows, F), aper=aper.view(rows, F),
                t_lag=t_lag.view(rows, F), t_period=t_period.view(rows, F), t_aper=t_aper.view(rows, F), t_power=t_power.view(rows, F))
    return {key: value.cpu().numpy() for key, value in host.items()}


# ----------------------------------------------------------------------------------------------------------------- the kernels
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_difference(shape):
    rows, n, W, L, hop, _ = shape
    want_d, want_p = _reference(shape)
    bound = R.dist_bound(W)
    for aligned in (True, False):
        got = _run(shape, aligned)
        d, power = got["d"].astype(np.float64), got["power"].astype(np.float64)
        err_d = np.abs(d - want_d) / np.maximum(want_d, 1e-300)
        err_p = np.abs(power - want_p) / np.maximum(want_p, 1e-300)
        print(f"{'aligned' if aligned else 'one float off'}: {d.shape[1]} frames; worst error of d {err_d.max():.3g}, of the power {err_p.max():.3g}, relative "
              f"(bound {bound:.3g}); exact zeros in d {int((d == 0).sum())} ({rows * d.shape[1]} at lag 0)")
        assert d.shape == want_d.shape and np.isfinite(d).all() and (d >= 0).all()
        assert (d[:, :, 0] == 0.0).all()                                                   # d(0) = 0 exactly
        assert (np.abs(d - want_d) <= bound * want_d).all()
        assert (np.abs(power - want_p) <= bound * want_p).all()
    assert np.array_equal(_run(shape, True)["d"], _run(shape, False)["d"]) and np.array_equal(_run(shape, True)["power"], _run(shape, False)["power"])
    if rows >= 3:                                                                          # the all-zero row: exact zeros throughout
        assert (_run(shape, True)["d"][rows - 1] == 0).all() and (_run(shape, True)["power"][rows - 1] == 0).all()


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_pick_on_the_devices_own_d(shape):
    rows, n, W, L, hop, tau_min = shape
    ambiguous_frames, fallback = 0, 0
    for aligned in (True, False):
        got = _run(shape, aligned)
        for r in range(rows):
            lag, period, aper, ambiguous = R.pick(got["d"][r].astype(np.float64), tau_min, THRESHOLD)
            ambiguous_frames += int(ambiguous.sum())
            fallback += int((aper >= THRESHOLD).sum())
            keep = ~ambiguous
            assert np.array_equal(got["lag"][r][keep], lag[keep]), (aligned, r)
            assert (np.abs(got["period"][r][keep] - period[keep]) <= 1e-12 * np.abs(period[keep])).all(), (aligned, r)
            assert (np.abs(got["aper"][r][keep] - aper[keep]) <= 1e-12 * np.abs(aper[keep])).all(), (aligned, r)
            assert ((got["lag"][r] >= tau_min) & (got["lag"][r] <= L - 2)).all()
            assert (np.abs(got["period"][r] - got["lag"][r]) <= 1.0).all()
    print(f"ambiguous frames: {ambiguous_frames} (must be 0); frames decided by the argmin, nothing under the threshold: {fallback}")
    assert ambiguous_frames == 0
    if rows >= 3:                                                                          # the all-zero row: S = 0, c = 1, the lowest lag of the range
        zero = _run(shape, True)
        assert (zero["lag"][rows - 1] == tau_min).all() and (zero["period"][rows - 1] == tau_min).all() and (zero["aper"][rows - 1] == 1.0).all()
    if rows >= 2:                                                                          # the noise row: the fallback argmin decides
        noise = rows - 2 if rows >= 3 else rows - 1
        assert (_run(shape, True)["aper"][noise] >= THRESHOLD).all()


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_track_is_pick_after_difference_bit_for_bit(shape):
    for aligned in (True, False):
        got = _run(shape, aligned)
        for key in ("lag", "period", "aper", "power"):
            a, b = torch.from_numpy(got["t_" + key]), torch.from_numpy(got[key])
            assert a.dtype == b.dtype and torch.equal(a, b), (key, aligned)
    for key in ("t_lag", "t_period", "t_aper", "t_power"):                                # the two placements: the same bits
        assert np.array_equal(_run(shape, True)[key], _run(shape, False)[key]), key


# ----------------------------------------------------------------------------------------------------------------- the Python layer
NOTE_PITCHES = [24, 36, 55, 60, 72, 84, 43, 67]


def test_python_layer_on_synthetic_notes():
    """Eight synthetic notes of 64000 samples through pitch.track and note_statistics: accurate, within 10 cents, and within 0.01 cent of the
    all-float64 restatement's median (what a perturbation of d by its fp32 bound moves a median by, measured in tests/test_yin_cpu.py: about
    0.001 cent -- times eight)."""
    from gansynth_amd import kernels, metrics, pitch, spectral_ops
    waves = torch.from_numpy(np.stack([R.synthetic_note(p) for p in NOTE_PITCHES])).cuda()
    t = pitch.track(waves)
    assert t.lag.dtype == torch.int32 and t.period.dtype == torch.float64 and t.aperiodicity.dtype == torch.float64 and t.power.dtype == torch.float32
    assert all(x.shape == (8, 245) and x.is_cuda for x in t)
    stats = pitch.note_statistics(t.period, t.aperiodicity, t.power, NOTE_PITCHES)
    for i, p in enumerate(NOTE_PITCHES):
        d, power = R.synthetic_tracks(p)
        _, period, aper, _ = R.pick(d)
        want, _, voiced = R.note(period, aper, power, p)
        print(f"pitch {p}: median {stats.cents[i]:+.4f} cents (float64 restatement {want:+.4f}, apart {abs(stats.cents[i] - want):.6f}), jitter "
              f"{stats.jitter[i]:.4f}, voiced {stats.voiced[i]} (restatement {voiced})")
        assert abs(stats.cents[i]) < 10.0 and abs(stats.cents[i] - want) < 0.01
    figures = pitch.summarize(stats.cents, stats.jitter)
    assert figures["f0_pitch_accuracy"] == 1.0 and figures["f0_chroma_accuracy"] == 1.0 and figures["f0_voiced_fraction"] == 1.0
    details = {}
    assert metrics.f0_pitch_accuracy_device(waves.cpu().numpy(), NOTE_PITCHES, details=details) == figures
    assert np.array_equal(details["cents"], stats.cents) and np.array_equal(details["voiced"], stats.voiced)
    # the wrappers: the same bits as one another, views with row slack are taken as they stand
    d, power = kernels.yin_difference(waves, 1024, 512, 256)
    lag, period, aper = kernels.yin_pick(d, 8, 0.15)
    assert torch.equal(lag, t.lag) and torch.equal(period, t.period) and torch.equal(aper, t.aperiodicity) and torch.equal(power, t.power)
    slack = torch.full((8, 64003), float("nan"), device="cuda")
    slack[:, :64000] = waves
    assert torch.equal(pitch.track(slack[:, :64000]).period, t.period)
    f0, aperiodicity = spectral_ops.estimate_f0(waves)
    assert f0.shape == (8, 245) and f0.dtype == torch.float64 and torch.equal(aperiodicity, t.aperiodicity)
    voiced = ~torch.isnan(f0)
    assert torch.equal(f0[voiced], 16000.0 / t.period[voiced]) and int(voiced.sum()) == int(stats.voiced.sum())
    one, _ = spectral_ops.estimate_f0(waves[3])
    assert one.shape == (245,) and torch.equal(one[~torch.isnan(one)], f0[3][~torch.isnan(f0[3])])
    with pytest.raises(ValueError, match="x must be on the HIP device"):
        pitch.track(waves.cpu())


# ----------------------------------------------------------------------------------------------------------------- evaluate and the driver
F0_KEYS = {prefix + key for prefix in ("", "real_") for key in ("f0_pitch_accuracy", "f0_chroma_accuracy", "f0_median_abs_cents", "f0_jitter_cents",
                                                                "f0_voiced_fraction")}


def test_evaluate_with_f0(tmp_path, gpu_store):
    from gansynth_amd import checkpoint
    from tests.test_classifier_gpu import _gan
    outs, extra = {}, {}
    for mode in ("swd", "f0", "both"):
        model = _gan(8, 2)                                     # 16 notes per side
        model._ensure_built(torch.randn(8, 256, device="cuda"), torch.eye(61, device="cuda")[:8])
        if mode == "swd":
            checkpoint.save(model, str(tmp_path))
        extra[mode] = {}
        kw = dict(swd=True) if mode == "swd" else dict(f0=True) if mode == "f0" else dict(swd=True, f0=True)
        outs[mode] = model.evaluate(str(tmp_path), None, None, "images:0", ["features:0", "logits:0"], features_out=extra[mode], **kw)
        print(mode, outs[mode])
    swd_keys = {"sliced_wasserstein_distance", "sliced_wasserstein_distance_levels"}
    assert set(outs["swd"]) == swd_keys and set(outs["f0"]) == F0_KEYS and set(outs["both"]) == swd_keys | F0_KEYS   # without f0: the keys as before
    assert all(outs["both"][key] == outs["swd"][key] for key in swd_keys)
    out = outs["f0"]
    assert all(isinstance(out[key], float) for key in F0_KEYS)
    assert out["real_f0_pitch_accuracy"] == 1.0 and out["real_f0_voiced_fraction"] == 1.0 and out["real_f0_chroma_accuracy"] == 1.0
    assert np.isfinite(out["real_f0_median_abs_cents"]) and out["real_f0_median_abs_cents"] < 10.0 and np.isfinite(out["real_f0_jitter_cents"])
    for key in ("f0_pitch_accuracy", "f0_chroma_accuracy", "f0_voiced_fraction"):
        assert 0.0 <= out[key] <= 1.0
    assert out["f0_pitch_accuracy"] <= out["f0_chroma_accuracy"] <= out["f0_voiced_fraction"]
    for key in ("f0_median_abs_cents", "f0_jitter_cents"):                                 # defined over the accurate notes: NaN only without one
        assert np.isnan(out[key]) == (out["f0_pitch_accuracy"] == 0.0)
    assert all(outs["both"][key] == out[key] or (np.isnan(outs["both"][key]) and np.isnan(out[key])) for key in F0_KEYS)
    for name in ("real_f0_cents", "fake_f0_cents"):
        assert extra["f0"][name].shape == (16,) and extra["f0"][name].dtype == np.float64 and name not in extra["swd"]
    assert not np.isnan(extra["f0"]["real_f0_cents"]).any()
    assert int((~np.isnan(extra["f0"]["fake_f0_cents"])).sum()) == round(out["f0_voiced_fraction"] * 16)
    with pytest.raises(ValueError, match="classifier=None needs swd=True or f0=True"):
        model.evaluate(str(tmp_path), None, None)
    with pytest.raises(ValueError, match="label columns"):
        _gan(8, 1).evaluate(str(tmp_path), None, None, f0=True, pitches=range(24, 84))


def test_gan_synth_main_f0(tmp_path):
    cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "gan_synth_main.py"), "--evaluate", "--f0", "--classifier", "none", "--synthetic",
           "--model_dir", str(tmp_path / "model"), "--batch_size", "8", "--num_generate_batches", "2"]
    r = subprocess.run(cmd, cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    line = [s for s in r.stdout.splitlines() if "f0_pitch_accuracy" in s][-1]
    print(line)
    assert all(f"'{key}'" in line for key in F0_KEYS) and "frechet" not in line and "sliced" not in line
