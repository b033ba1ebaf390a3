"""GPU: gs_true_peak (gansynth_amd/csrc/true_peak.hip) element-wise against the float64 restatement of tests/true_peak_ref.py, every e[t]
within the resampler's bound (resample_ref.bound: (taps + 3) * 2^-24 * sum |T||x|, the largest among its terms); gs_limit_env against the
restatement fed the kernel's own fp32 envelope, held to exactly what tests/test_limiter_gpu.py holds gs_limit to (4 times the error of the
single-precision restatement, LR.FACTOR, and the same bit-exact properties); then the Python layers and the driver's --true_peak.
Every figure is printed before it is asserted."""
import functools
import json

import numpy as np
import pytest
import torch

from tests import limiter_ref as LR
from tests import true_peak_ref as TR

pytestmark = pytest.mark.gpu
T = TR.TILE
LT = LR.T
SENTINEL, PCM_SENTINEL, PAD = 12345.0, 77, 64
LENGTHS = (1, 33, 34, 35, 67, 68, 69, T - 1, T, T + 1, 2 * T + 35, 3 * T + 5)


def _K():
    from gansynth_amd import kernels
    return kernels.get()


def _table():
    return _K().resample_design(1, 4, "cuda")[1]


def spike_positions(n):
    """0, n - 1, both sides of every tile seam, and 33 / 34 samples either side of a seam: where a halo can go wrong."""
    at = {0, n - 1}
    for seam in range(T, n + 40, T):
        at |= {seam - 1, seam, seam - 33, seam - 34, seam + 33, seam + 34, seam - 35, seam + 32}
    return sorted(p for p in at if 0 <= p < n)


@functools.lru_cache(maxsize=None)
def _clip(rows, n):
    """Noise plus distinct spikes (a spike in row 0 or in row 1 alone, alternating), with its float64 envelope and bound: computed once, never
    written to."""
    g = np.random.Generator(np.random.PCG64(n * 31 + rows))
    x = g.uniform(-0.4, 0.4, (rows, n)).astype(np.float32)
    for k, p in enumerate(spike_positions(n)):
        x[k % rows, p] = np.float32((1.0 + 0.05 * k) * (-1) ** k)
    e, bound = TR.detector(x)
    for arr in (x, e, bound):
        arr.setflags(write=False)
    return x, e, bound


def _detect(x, aligned=True, slack=0, want_env=True, want_peak=True):
    """gs_true_peak itself on x [rows, n]: rows `n + slack` apart inside a buffer that is NaN everywhere else (so nothing outside [0, n) may
    be read as a sample), env inside a buffer full of a sentinel.  `aligned`: x and env on 16 bytes, else one float off.  -> (env [n] or None,
    peak or None) on the host; nothing outside env was written."""
    from gansynth_amd import kernels
    lib = _K().lib
    rows, n = x.shape
    off = 0 if aligned else 1
    stride = n + slack
    xbuf = torch.full((PAD + off + rows * stride + PAD,), float("nan"), device="cuda")
    xv = xbuf[PAD + off:PAD + off + rows * stride].view(rows, stride)
    xv[:, :n] = torch.tensor(x, device="cuda")
    ebuf = torch.full((PAD + off + n + PAD,), SENTINEL, device="cuda") if want_env else None
    peak = torch.full((1,), -1.0, device="cuda") if want_peak else None
    ws = torch.empty(max(int(lib.gs_true_peak_workspace_bytes(rows, n)), 16), dtype=torch.uint8, device="cuda")
    assert (xv.data_ptr() % 16 == 0) == aligned
    code = lib.gs_true_peak(_table().data_ptr(), xv.data_ptr(), rows, n, stride, None if ebuf is None else ebuf[PAD + off:].data_ptr(),
                            None if peak is None else peak.data_ptr(), ws.data_ptr(), ws.numel(), kernels._stream())
    torch.cuda.synchronize()
    assert code == 0, lib.gs_last_error()
    env = None
    if want_env:
        assert (ebuf[:PAD + off] == SENTINEL).all() and (ebuf[PAD + off + n:] == SENTINEL).all()
        env = ebuf[PAD + off:PAD + off + n].cpu().numpy()
    return env, (None if peak is None else float(peak))


@pytest.mark.parametrize("slack", [0, 3], ids=["stride n", "stride n+3"])
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "off16"])
@pytest.mark.parametrize("rows", [1, 2])
@pytest.mark.parametrize("n", LENGTHS)
def test_detector_against_the_restatement(n, rows, aligned, slack):
    x, e, bound = _clip(rows, n)
    env, peak = _detect(x, aligned, slack)
    err = np.abs(env.astype(np.float64) - e)
    worst = int(np.argmax(err - bound))
    print(f"n {n} rows {rows} {'aligned' if aligned else 'off16'} stride n+{slack}: largest error {err.max():.3g}, closest to its bound at t = {worst}: "
          f"{err[worst]:.3g} against {bound[worst]:.3g}; peak {peak:.6f} against {e.max():.6f}")
    assert env.dtype == np.float32 and not np.isnan(env).any()
    assert (err <= bound).all()
    assert (env >= np.abs(x).max(axis=0)).all()                                    # |x| itself is in the maximum, exactly
    assert np.float32(peak) == env.max()                                           # the exact fold of the computed e
    again = _detect(x, aligned, slack)                                             # two calls: bit-identical
    assert np.array_equal(again[0].view(np.uint32), env.view(np.uint32)) and again[1] == peak
    only_peak = _detect(x, aligned, slack, want_env=False)                         # either output left out
    only_env = _detect(x, aligned, slack, want_peak=False)
    assert only_peak == (None, peak) and only_env[1] is None and np.array_equal(only_env[0].view(np.uint32), env.view(np.uint32))


def test_detector_reads_the_crest_and_silence():
    from gansynth_amd import true_peak
    for period, phase in ((4, np.pi / 4), (8, np.pi / 8)):
        x = TR.sine(period, phase, 1.7).astype(np.float32)
        got = true_peak.measure(torch.tensor(x[0], device="cuda"))
        inner = _detect(x)[0][4 * TR.TAPS:-4 * TR.TAPS].max()
        print(f"period {period}: {TR.db(inner / 1.7):+.6f} dB from the amplitude inside, the whole clip {got:.4f} dBTP")
        assert abs(TR.db(inner / 1.7)) <= 0.01 and got >= TR.db(1.7) - 0.01
    assert true_peak.measure(torch.zeros(2, 5000, device="cuda")) == -np.inf
    stereo = torch.tensor(_clip(2, 3 * T + 5)[0], device="cuda")
    env, peak = _K().true_peak(stereo)
    assert env.shape == (3 * T + 5,) and peak.shape == (1,) and float(peak) == float(env.max())
    assert np.array_equal(env.cpu().numpy(), _detect(_clip(2, 3 * T + 5)[0])[0])
    none, alone = _K().true_peak(stereo[:, 1:-1], want_envelope=False)             # a view whose rows are off 16 bytes and 2 floats apart
    assert none is None and float(alone) == _detect(_clip(2, 3 * T + 5)[0][:, 1:-1].copy())[1]
    with pytest.raises(ValueError, match="must be on the HIP device"):
        _K().true_peak(stereo.cpu())


# ------------------------------------------------------------------------------------------------------------------- gs_limit_env
C, D = LR.C, LR.D


def _limit(x, env, d, c, W, aligned, want_pcm=True, want_stats=True, env_offset=None):
    """tests/test_limiter_gpu.py's _run for gs_limit_env (env: [n] fp32 on the host, moved off 16 bytes with a single row of x, or by
    `env_offset` floats) or, with env None, for gs_limit."""
    from gansynth_amd import kernels
    lib = _K().lib
    rows, n = x.shape
    offset = 1 if (rows == 1 and not aligned) else 0
    stride = (n + 7) // 4 * 4 + (0 if aligned else 1)
    xbuf = torch.full((offset + rows * stride,), float("nan"), device="cuda")
    xv = xbuf[offset:].view(rows, stride)
    xv[:, :n] = torch.tensor(x, device="cuda")
    ev = None
    if env is not None:
        eo = offset if env_offset is None else env_offset
        ebuf = torch.full((eo + n + 4,), float("nan"), device="cuda")
        ev = ebuf[eo:eo + n]
        ev[:] = torch.tensor(env, device="cuda")
    buf = torch.full((PAD + offset + rows * stride + PAD,), SENTINEL, dtype=torch.float32, device="cuda")
    out = buf[PAD + offset:PAD + offset + rows * stride].view(rows, stride)
    pbuf = torch.full((PAD + rows * n + PAD,), PCM_SENTINEL, dtype=torch.int16, device="cuda") if want_pcm else None
    peak = torch.full((1,), -1.0, device="cuda") if want_stats else None
    gain = torch.full((1,), -1.0, device="cuda") if want_stats else None
    ws = torch.empty(max(int(lib.gs_limit_workspace_bytes(rows, n)), 16), dtype=torch.uint8, device="cuda")
    tail = (rows, n, stride, float(d), float(c), int(W), out.data_ptr(), stride, None if pbuf is None else pbuf[PAD:].data_ptr(),
            None if peak is None else peak.data_ptr(), None if gain is None else gain.data_ptr(), ws.data_ptr(), ws.numel(), kernels._stream())
    code = lib.gs_limit(xv.data_ptr(), *tail) if env is None else lib.gs_limit_env(xv.data_ptr(), ev.data_ptr(), *tail)
    torch.cuda.synchronize()
    assert code == 0, lib.gs_last_error()
    assert (buf[:PAD + offset] == SENTINEL).all() and (buf[PAD + offset + rows * stride:] == SENTINEL).all()
    assert (out[:, n:] == SENTINEL).all()
    pcm = None
    if want_pcm:
        assert (pbuf[:PAD] == PCM_SENTINEL).all() and (pbuf[PAD + rows * n:] == PCM_SENTINEL).all()
        pcm = pbuf[PAD:PAD + rows * n].cpu().numpy()
        pcm = pcm if rows == 1 else pcm.reshape(n, rows)
    return out[:, :n].cpu().numpy(), pcm, (None if peak is None else float(peak)), (None if gain is None else float(gain))


def _exact(out, pcm, peak, gain, y, scaled_env, c, W):
    """tests/test_limiter_gpu.py's _exact, `quiet` taken with the envelope: the properties that hold bit for bit."""
    c = np.float32(c)
    assert out.dtype == np.float32 and out.shape == y.shape and not np.isnan(out).any()
    assert (np.abs(out) <= c).all()
    quiet = np.broadcast_to(TR.quiet(y, scaled_env, c, W)[None, :], y.shape)
    assert np.array_equal(out[quiet].view(np.uint32), y[quiet].view(np.uint32))
    assert np.array_equal(pcm, LR.pcm(out))
    assert np.float32(peak) == LR.peak(out)
    assert 0 < gain <= 1
    least = np.abs((np.float32(gain) * y).astype(np.float32))
    free = np.abs(out) < c
    assert (least[free] <= np.abs(out)[free]).all()
    assert gain == 1 or (np.minimum(least, c) == np.abs(out)).any()


@functools.lru_cache(maxsize=None)
def _limit_case(n, rows, W, k):
    """Draw k of a case: LR.draw's clip, the fp32 envelope THE DETECTOR KERNEL gives for it (so the two kernels' errors are not stacked), and
    the two restatements fed that envelope.  Computed once, never written to."""
    x = LR.draw(n, rows, W, k=k)
    env = _detect(x)[0]
    y, scaled = LR.pre(x, D), TR.scaled_envelope(env, D)
    ref, f32 = TR.limit_f64(y, scaled, C, W), TR.limit_f32(y, scaled, C, W)
    for arr in (x, env, y, scaled) + tuple(ref) + tuple(f32):
        arr.setflags(write=False)
    return x, env, y, scaled, ref, f32


@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "off16"])
@pytest.mark.parametrize("rows", [1, 2])
@pytest.mark.parametrize("W,n", [(W, n) for W in (1, 64, 240, 257, 2048) for n in (W, LT + 1, 3 * LT + 5)], ids=lambda v: str(v))
def test_limit_env_against_the_restatement(W, n, rows, aligned):
    e_out = e_g = b_out = b_g = 0.0
    louder = 0
    for k in range(LR.draws(n)):
        x, env, y, scaled, ref, f32 = _limit_case(n, rows, W, k)
        out, pcm, peak, gain = _limit(x, env, D, C, W, aligned)
        _exact(out, pcm, peak, gain, y, scaled, C, W)
        e_out, b_out = max(e_out, LR.out_error(out, ref)), max(b_out, LR.out_error(f32.out, ref))
        e_g, b_g = max(e_g, LR.gain_error(out, ref, C, gain)), max(b_g, LR.gain_error(f32.out, ref, C, f32.g.min()))
        louder += int((scaled > LR._envelope(y)).sum())
        if k == 0:
            again = _limit(x, env, D, C, W, aligned)
            assert np.array_equal(again[0].view(np.uint32), out.view(np.uint32)) and np.array_equal(again[1], pcm) and again[2:] == (peak, gain)
    print(f"W {W} n {n} rows {rows} {'aligned' if aligned else 'off16'} ({LR.draws(n)} draws, the envelope above the samples at {louder} of them): "
          f"out {e_out:.3g} against limit_f32's {b_out:.3g}, g {e_g:.3g} against {b_g:.3g}")
    assert e_out <= LR.FACTOR * b_out and e_g <= LR.FACTOR * b_g
    assert louder > 0 or n == 1                                                     # the envelope takes part


@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "off16"])
@pytest.mark.parametrize("rows", [1, 2])
def test_limit_env_with_the_sample_envelope_is_gs_limit(rows, aligned):
    for W, n in ((240, 3 * LT + 5), (2048, LT + 1), (1, 1)):
        x = LR.draw(n, rows, W)
        plain = _limit(x, None, D, C, W, aligned)
        same = _limit(x, np.abs(x).max(axis=0), D, C, W, aligned)
        assert np.array_equal(plain[0].view(np.uint32), same[0].view(np.uint32)) and np.array_equal(plain[1], same[1]) and plain[2:] == same[2:]
        moved = _limit(x, np.abs(x).max(axis=0), D, C, W, aligned, env_offset=3)                      # env alone off 16 bytes
        assert np.array_equal(plain[0].view(np.uint32), moved[0].view(np.uint32)) and np.array_equal(plain[1], moved[1]) and plain[2:] == moved[2:]
    only = _limit(x, np.abs(x).max(axis=0), D, C, W, aligned, want_pcm=False, want_stats=False)     # the optional outputs left out
    assert only[1:] == (None, None, None) and np.array_equal(only[0], plain[0])
    x = LR.draw(LT + 1, rows, 64)
    holed = np.abs(x).max(axis=0)
    holed[::7] = np.nan                                                               # a NaN in the envelope contributes nothing
    assert np.array_equal(_limit(x, holed, D, C, 64, aligned)[0], _limit(x, None, D, C, 64, aligned)[0])


# --------------------------------------------------------------------------------------------------------------- the Python layer
def test_the_feature_bites():
    """The fs/4 sine at 45 degrees, amplitude 2, n = 8192, through limiter.apply at -1 dB, W = 240: with true_peak the output's true peak is at
    most -1 + 0.05 dBTP; without, more than -1 + 2.5 (analysis: +3.01).  drive 0 with true_peak: the gain 1 throughout, out = fl(d * x) bit
    for bit, and its true peak at or under the ceiling up to the detector's bound."""
    from gansynth_amd import kernels, limiter, true_peak
    x = TR.inputs()["sine"].astype(np.float32)[0]
    clip = torch.tensor(x, device="cuda")
    assert limiter.lookahead_samples(48000, 0.005) == 240
    out, pcm, peak, gain = limiter.apply(clip, 48000, ceiling_db=-1.0, want_pcm=True, true_peak=True)
    held = true_peak.measure(out)
    plain = limiter.apply(clip, 48000, ceiling_db=-1.0, want_pcm=True)
    loose = true_peak.measure(plain[0])
    c = np.float32(10.0 ** (-1 / 20))
    print(f"true peak of the limited sine: {held:+.4f} dBTP with true_peak, {loose:+.4f} dBTP without; sample peaks {float(peak):.6f} and {float(plain[2]):.6f}, "
          f"least gains {float(gain):.4f} and {float(plain[3]):.4f}")
    assert held <= -1.0 + 0.05
    assert loose > -1.0 + 2.5
    assert float(peak) <= c and float(plain[2]) <= c and float(gain) < float(plain[3]) < 1
    assert np.array_equal(pcm.cpu().numpy(), LR.pcm(out.cpu().numpy()))
    # what apply did: the detector's envelope and true peak into design and kernels.limit
    env, tp = kernels.true_peak(clip)
    d, cc, w = limiter.design(48000, -1.0, 6.0, 0.005, float(tp))
    want = kernels.limit(clip, d, cc, w, want_pcm=True, envelope=env)
    assert all(torch.equal(a, b) for a, b in zip((out, pcm, peak, gain), want))
    # drive 0: only scaled
    flat, _, flat_peak, flat_gain = limiter.apply(clip, 48000, ceiling_db=-1.0, drive_db=0.0, true_peak=True)
    d0 = limiter.design(48000, -1.0, 0.0, 0.005, float(tp))[0]
    assert float(flat_gain) == 1.0
    assert np.array_equal(flat.cpu().numpy().view(np.uint32), LR.pre(x, d0)[0].view(np.uint32))
    e, bound = TR.detector(LR.pre(x, d0))
    print(f"drive 0: true peak {true_peak.measure(flat):+.5f} dBTP, {10 ** (true_peak.measure(flat) / 20) - float(c):+.3g} from the ceiling (bound {bound.max():.3g})")
    assert 10 ** (true_peak.measure(flat) / 20) <= float(c) + 2 * bound.max()
    # stereo through loudness.apply: the envelope goes to the limiter there too
    from gansynth_amd import loudness
    two = torch.tensor(np.stack([x, 0.5 * x]).astype(np.float32), device="cuda").repeat(1, 6)
    hot, _, info = loudness.apply(two, 48000, 3.0, true_peak=True)                  # (about 4 dB down: the samples under the ceiling, the crests not)
    hot_plain, _, info_plain = loudness.apply(two, 48000, 3.0)
    print(f"loudness.apply at +3 LUFS from {info['measured_lufs']:.2f}: {true_peak.measure(hot):+.4f} dBTP with true_peak (least gain {info['min_gain']:.4f}), "
          f"{true_peak.measure(hot_plain):+.4f} without ({info_plain['min_gain']:.4f})")
    assert true_peak.measure(hot) <= -1.0 + 0.05 < true_peak.measure(hot_plain) and info["min_gain"] < 1 and info["min_gain"] <= info_plain["min_gain"]


# ---------------------------------------------------------------------------------------------------------------------- the driver
def test_driver_true_peak(gpu_store, tmp_path):
    """`gan_synth_main.py --synthesize score.json --stereo --output_rate 48000 --limit -1 --true_peak`, and the same with `--loudness -16`:
    the reported true peak is at most -1 + 0.05 dBTP and no PCM sample is above the ceiling; without the flag the file is byte for byte the
    one limiter.apply / loudness.apply write with their defaults, and reports no true peak."""
    from scipy.io import wavfile
    import gan_synth_main as main
    from gansynth_amd import limiter, loudness
    from tests.test_limiter_gpu import _four_notes
    from tests.test_notes_gpu import _model
    model = _model()
    (tmp_path / "score.json").write_text(json.dumps(_four_notes()))
    common = ["--synthesize", str(tmp_path / "score.json"), "--batch_size", "4", "--release_seconds", "0.01", "--model_dir", str(tmp_path / "no_model"),
              "--seed", "3", "--stereo", "--output_rate", "48000"]
    c = 10.0 ** (-1.0 / 20)
    lines = []

    def render(name, extra):
        args = main.parser.parse_args(common + ["--output", str(tmp_path / name)] + extra)
        info = main.synthesize_to_wav(model, args, range(24, 85), log=lines.append)
        rate, data = wavfile.read(str(tmp_path / name))
        assert rate == 48000 and data.dtype == np.int16 and data.ndim == 2 and data.shape[1] == 2
        return info, data

    clip = model.synthesize(str(tmp_path / "score.json"), normalize=False, sample_rate=48000, stereo=True, batch_size=4, release_seconds=0.01, seed=3)
    for name, flags in (("limit", ["--limit", "-1"]), ("loudness", ["--loudness", "-16"])):
        info, data = render(name + "_tp.wav", flags + ["--true_peak"])
        plain_info, plain = render(name + ".wav", flags)
        written = [line for line in lines if "written to" in line]
        print(f"driver {' '.join(flags)} --true_peak: {info['true_peak_db']:+.4f} dBTP, largest |pcm| {np.abs(data.astype(np.int64)).max()} against "
              f"round(c * 32768) = {round(c * 32768)}, least gain {info['limit_min_gain']:.4f} ({plain_info['limit_min_gain']:.4f} without the flag)")
        assert info["true_peak_db"] <= -1.0 + 0.05
        assert np.abs(data.astype(np.int64)).max() <= round(c * 32768) and info["limit_peak"] <= np.float32(c)
        assert "dBTP" in written[-2] and f"true peak {info['true_peak_db']:.2f} dBTP" in written[-2]
        assert "true_peak_db" not in plain_info and "dBTP" not in written[-1]
        assert info["limit_min_gain"] <= plain_info["limit_min_gain"]
        if name == "limit":
            pcm = limiter.apply(clip, 48000, ceiling_db=-1.0, drive_db=6.0, lookahead_seconds=0.005, peak=plain_info["peak"], want_pcm=True)[1]
        else:
            pcm = loudness.apply(clip, 48000, -16.0, ceiling_db=-1.0, lookahead_seconds=0.005, want_pcm=True)[1]
        assert np.array_equal(plain, pcm.cpu().numpy())
